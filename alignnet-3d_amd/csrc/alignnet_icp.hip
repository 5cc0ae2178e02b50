// ICP refinement of the network's prediction on the FULL clouds, gfx950 only.
//
// Replaces icp.icp_p2point (reference icp.py:69-78: o3.registration_icp with
// TransformationEstimationPointToPoint(with_constraint=True, with_scaling=False)) as called from the evaluation loop
// (train.py:463-484: radius 0.1, `--its` iterations, init = get_mat_angle(prediction)).  Open3D (a private fork,
// README.md:32) is not part of the reference tree; the loop and the z-constrained point-to-point estimate are
// restated in oracle/icp_ref.py, which this kernel follows step for step (same order of evaluate / estimate / stop).
//
// One workgroup per pair, all arithmetic in fp64 (Open3D computes in double; nearest-neighbour decisions then agree
// with the oracle).  The target cloud sits in LDS as doubles (structure of arrays: no conversion in the inner loop),
// the source cloud is re-read from HBM/L2 each iteration (a few thousand points).  Brute force n1 x n2 per
// iteration: at the cloud sizes this scan was built for (about 1,500 points: a few million distance evaluations per pair, every target in the LDS
// stage) a search structure would be slower to build than this is to run.  That stops holding where the scan leaves its LDS stage (4266 targets:
// everything beyond is an all-fp64 walk from L2, in every iteration, for every source point) -- the scene generator's clouds have 2,000 to 58,600
// points -- and there the GRID search below takes over when alignnet_set_option "icp_search" asks for it (1: every pair, 2: pairs above that size).
// Round 6: sixteen waves per pair instead of four, and FOUR LANES PER SOURCE POINT (lane s of a quad scans targets s, s + 4, ...; the
// quad's (distance, index) minima meet in two shuffles, equal distances going to the lower index = the oracle's argmin): 256 pairs x 256
// threads put one wave on every SIMD and 1500 points on 256 threads (six rounds of a serial 1500-long scan each); now a CU holds four
// waves per SIMD and a scan is 375 long.
// And the scan is CERTIFIED in fp32 before it is decided in fp64: one pass takes, per lane, the smallest and second smallest fp32 distance of its slice
// (packed arithmetic, two targets per instruction) and where the smallest sits; the quad's minimum m gives a threshold m + 4 eps with
// eps >= |fp32 distance - exact distance| for every target that can matter (icp_prefilter_eps: the rounding of the transformed source point to fp32, of
// the differences, of the three products and sums).  Any target whose fp64 distance equals the minimum has an fp32 distance under the threshold, so: a
// lane whose smallest is under it and whose second smallest is not evaluates that ONE target in fp64 (the old arithmetic); a lane with two or more under
// it (a near-tie inside its slice: rare) walks its slice in fp64 as before; the quad's (distance, index) minima meet as before.  Same decisions as the
// all-fp64 scan at a third of its vector-issue time (a first form with the fp64 evaluation inside the scan loop spilled around the branch: 7.7 ms).
// icp_kernel<kFull>: the estimate kind.  kFull = false is the z-constrained estimate above (with_constraint=True).  kFull = true is Open3D's
// unconstrained point-to-point estimate (with_constraint=False: Eigen::umeyama(src, dst, false) over the inlier correspondences), used by the
// ICP baseline evaluation mode (icp.py:150-213): the same scan, 17 sums instead of 10 (count, sum a, sum b, the nine entries of sum b a^T, sum of
// distances, all about the same pivot), then the 3x3 Umeyama rotation in fp64 on one lane (icp_umeyama_rotation: one-sided Jacobi SVD).
#include "engine.h"
#include "host_util.h"
#include "icp_estimate.h"
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

namespace {

constexpr int kIcpThreads = 1024, kIcpSums = 12, kIcpSplit = 4;   // threads per pair; sums of the z-constrained estimate; lanes per source point
constexpr int kIcpSumsFull = 19;     // sums of the full-rotation estimate: count, a (3), b (3), b a^T (9), distance, |a|^2, |b|^2
// A cross-covariance that is zero up to the rounding of its one-pass sums (one correspondence; every source point on the same target point) determines no
// rotation: the estimate then keeps the rotation (Eigen's SVD of a zero matrix and the oracle's atan2(0, 0) both give the identity) instead of reading an
// angle out of the residue (two source points on one target came out turned by pi).  Each entry is a sum of n products
// bounded, with its centring term, by (n + 4) u sqrt(sum |a|^2 sum |b|^2) of rounding (Cauchy-Schwarz on the products' magnitudes), u = 2^-53.
constexpr double kIcpNoise = 8.0 * 1.1102230246251565e-16;
constexpr float kIcpFar = 1e18f;      // padding of the fp32 slices: a distance of 3e36, under no threshold
typedef float icp_f32x2 __attribute__((ext_vector_type(2)));

// slice-major fp32 copy of the LDS-resident targets: lane s of a quad reads targets s, s + 4, ... as consecutive floats, two per 8-byte read
__host__ __device__ constexpr int icp_slice_len(int lds_points) { return (((lds_points + 3) / 4 + 1) & ~1) + 2; }
constexpr size_t icp_lds_bytes(int lds_points) { return (size_t)lds_points * 24 + (size_t)3 * kIcpSplit * icp_slice_len(lds_points) * 4; }

// eps >= |e32 - d| for a target at exact squared distance d <= M from a source point with |coordinates| <= P (u = 2^-24): the source point is rounded to
// fp32 (u P per coordinate), each difference once more (u (P + a) in all, a = |difference|), so a squared difference moves by <= 2 a u (P + a) + u^2 (P + a)^2,
// and the product and two fmas round the running sum three times (3 u d): eps = u (2 sqrt(3) P sqrt(d) + 5 d) + 3 u^2 (P + sqrt(d))^2.  Returned with room:
// 2^-23 (4 P sqrt(M) + 6 M) + 2^-44 (P + sqrt(M))^2.
__device__ __forceinline__ float icp_prefilter_eps(float P, float M)
{
  const float r = sqrtf(M);
  return 1.1920929e-7f * (4.f * P * r + 6.f * M) + 5.6843419e-14f * (P + r) * (P + r);
}

struct IcpArgs {
  const float* pts[2];          // point blobs
  const long long* off;         // [n + 1][2] row offsets into the blobs
  const int* rows;              // [B] example rows, or null: pair b is row b
  const double* init;           // [B][16] row-major 4x4
  double radius; int its;
  int lds_points;               // target points that fit in LDS
  double* out;                  // [B][16]
  double* fitness; double* rmse; int* iters;   // [B] each, may be null
  // read only by the traced instantiations (icp_kernel<kFull, true>, alignnet_debug_icp_scan: one pair): per source point of the FIRST evaluation
  int* tr_index; double* tr_dist; int* tr_inlier; int* tr_paths;
};

// ---- grid search (alignnet_set_option "icp_search"): a fixed-radius nearest-neighbour search on a uniform grid --------------------------------------
// ICP accepts a correspondence only within `radius`, so the nearest target that can count lies in the 27 cells around the query's cell when cells are
// at least one radius wide.  Per pair, once per call (icp_grid_build_kernel): the targets are bucket-sorted by hashed cell (count, exclusive scan,
// scatter) into float4 (x, y, z, original index) records behind a table of bucket starts -- H = icp_grid_buckets(n2) <= 32768 buckets whatever the
// cloud's extent (a hash of the integer cell coordinates, not a dense box: O(n2) memory; two cells in one bucket only ADD candidates).  The ICP
// kernel (icp_kernel<kFull, kTrace, true>) holds the table in LDS and reads the records from L2; ONE lane per source point walks the buckets of its 27
// cells and evaluates every record in fp64 exactly as the scan's fp64 step does, keeping the smallest (distance, original index) pair -- a minimum over
// a set, so neither the order inside a bucket (the scatter's atomics) nor visiting a bucket twice (two of the 27 cells hashing alike) can change it.
//
// Cell edge e = max(radius (1 + 2^-20), (M + radius) 2^-20), M = max |target coordinate| of the pair; cell(x) = clamp(floor(x / e), +-2^30), all fp64.
// Claim: a target the kernel accepts (fp64 distance d <= r2 = fl(radius^2)) differs from the query by at most one cell per axis.  With u = 2^-53: the
// three differences, squares and sums round d by <= 5 u d, r2 by u, so per axis |p - q| <= radius (1 + 4 u); both coordinates are <= M + radius (1 + 4 u)
// in magnitude, and each quotient x / e rounds once: the two computed quotients differ by <= [radius (1 + 4 u) + 2 u (M + 2 radius)] / e.  Where
// e = radius (1 + 2^-20) >= (M + radius) 2^-20, M <= 2^20 radius and the bracket is <= radius (1 + 4 u + 2^-32 + 2^-51) < e.  Where e = (M + radius) 2^-20
// > radius (1 + 2^-20): radius (1 + 4 u) < e (1 - 2^-21) and 2 u (M + 2 radius) <= 4 u 2^20 e = 2^-31 e, together < e.  (The roundings of e itself, 2 u,
// sit inside the 2^-21 of slack.)  Quotients that differ by <= 1 have floors that differ by <= 1, and the clamp is monotone.  (On 1.5 M random and
// planted float32 pairs within a radius of 0.1, cells exactly one radius wide lost none either, tests/test_icp_grid_cpu.py: the margin is what makes the
// claim hold for every radius and magnitude, not the cure of a loss seen.)
// Integer range: a target's |cell| <= M / e <= 2^20; a query anywhere (a far initial transform, a non-finite coordinate) is clamped to +-2^30 before the
// conversion, so cell +- 1 never overflows -- such a query meets whatever shares its buckets, all of it farther than the radius.  A radius below
// 2^-20 of the coordinates' magnitude is what enlarges e: cells wider than the radius stay correct, they only hold more candidates.
constexpr int kGridMinBuckets = 64, kGridMaxBuckets = 32768;   // the table (H + 1 ints) stays within 128 KiB + 4 of LDS
constexpr double kGridCellMax = 1073741824.0, kGridSpan = 9.5367431640625e-07;   // 2^30, 2^-20
constexpr size_t kIcpGridWsBudget = (size_t)1 << 30;   // workspace of one chunk of grid pairs
struct IcpGridInfo { double edge; int buckets, occupied, largest, pad; };   // per pair, at the head of its workspace

__host__ __device__ inline int icp_grid_buckets(long long n2)
{
  int H = kGridMinBuckets;
  while (H < n2 && H < kGridMaxBuckets) H <<= 1;
  return H;
}
// a pair's workspace: IcpGridInfo (256 bytes) | bucket starts [H + 1] ints | records [n2] float4
__host__ __device__ inline size_t icp_grid_table_bytes(long long n2) { return (((size_t)icp_grid_buckets(n2) + 1) * 4 + 255) & ~(size_t)255; }
__host__ __device__ inline size_t icp_grid_pair_bytes(long long n2) { return 256 + icp_grid_table_bytes(n2) + (((size_t)n2 * 16 + 255) & ~(size_t)255); }
__device__ __forceinline__ int icp_grid_cell(double x, double e)
{
  const double c = fmin(fmax(floor(x / e), -kGridCellMax), kGridCellMax);   // (fmax / fmin drop a NaN)
  return (int)c;
}
__device__ __forceinline__ unsigned icp_grid_hash(int cx, int cy, int cz)
{
  unsigned v = (unsigned)cx * 73856093u ^ (unsigned)cy * 19349663u ^ (unsigned)cz * 83492791u;
  v ^= v >> 15; v *= 0x2c1b3c6du; v ^= v >> 12;
  return v;
}
__device__ __forceinline__ unsigned icp_grid_bucket(double x, double y, double z, double e, unsigned mask)   // the bucket of a point
{
  return icp_grid_hash(icp_grid_cell(x, e), icp_grid_cell(y, e), icp_grid_cell(z, e)) & mask;
}

// one grid as the kernels address it, decoded from the pair's workspace `ws` (the layout above).  edge: the build's, read only from a built grid
struct IcpGridView { char* ws; int* start; float4* rec; unsigned mask; double edge; int buckets; };
__device__ __forceinline__ IcpGridView icp_grid_view(char* ws, long long n2, bool built = true)
{
  IcpGridView g;
  g.ws = ws;
  g.buckets = icp_grid_buckets(n2);
  g.start = reinterpret_cast<int*>(ws + 256);
  g.rec = reinterpret_cast<float4*>(ws + 256 + icp_grid_table_bytes(n2));
  g.mask = (unsigned)g.buckets - 1u;
  g.edge = built ? reinterpret_cast<const IcpGridInfo*>(ws)->edge : 0.0;
  return g;
}

// The search of one query (px, py, pz): every record in the buckets of the 27 cells around it, in fp64, into the smallest (distance, original index)
// pair seen so far (best, bj) and that record's coordinates (brec.x, .y, .z).  kCount (the traced instantiation): cand += the records evaluated.
// The minimum runs in scalars of this function and not in the caller's float4: that is what the kernels compiled to when the walk stood in them (as
// a 4-vector behind the reference the winner changed the schedule of the sums that follow the search, and which of their products were fused)
template <bool kCount>
__device__ __forceinline__ void icp_grid_nearest(double px, double py, double pz, const IcpGridView& g, double& best, int& bj, float4& brec, int& cand)
{
  double m = best; int mj = bj; float mx = brec.x, my = brec.y, mz = brec.z;
  const int gx = icp_grid_cell(px, g.edge), gy = icp_grid_cell(py, g.edge), gz = icp_grid_cell(pz, g.edge);
#pragma unroll 1
  for (int c = 0; c < 27; ++c) {
    const unsigned hb = icp_grid_hash(gx + c % 3 - 1, gy + (c / 3) % 3 - 1, gz + c / 9 - 1) & g.mask;
    const int lo = g.start[hb], hi = g.start[hb + 1];
#pragma unroll 1
    for (int j = lo; j < hi; ++j) {
      const float4 q = g.rec[j];
      const int oj = __float_as_int(q.w);
      const double ddx = px - (double)q.x, ddy = py - (double)q.y, ddz = pz - (double)q.z;
      const double d = ddx * ddx + ddy * ddy + ddz * ddz;
      if (d < m || (d == m && oj < mj)) { m = d; mj = oj; mx = q.x; my = q.y; mz = q.z; }   // equal distances: the lower original index
    }
    if constexpr (kCount) cand += hi - lo;   // candidates evaluated
  }
  best = m; bj = mj; brec.x = mx; brec.y = my; brec.z = mz;
}

struct IcpGridArgs : IcpArgs {
  char* ws;                     // the chunk's workspace
  const long long* ws_off;      // [B] byte offset of pair b's part
};

// alignnet_evaluate_registration*: ONE evaluation at the given transform (icp_kernel<false, false, kGrid, true>) and, over its inliers, the sums of
// Open3D's GetInformationMatrixFromPointClouds.  With (x, y, z) = the inlier's TARGET point minus the pair's centre, G^T G of the three rows
// [0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1] has 21 upper entries of which six are zero, three are the count and the other twelve are
// nine distinct sums and their negatives: eleven accumulators with the count and the squared distances (kIcpSumsEval), fixed order, mirrored at the end
struct IcpEvalArgs : IcpGridArgs {
  const double* centers;        // [B][3], or null: the origin
  double* info;                 // [B][36] row-major, or null: the sums are not taken
  int* corr;                    // per source point the inlier's target (original index) or -1, or null
  const long long* corr_off;    // [B] where pair b's source range starts in corr
};
constexpr int kIcpSumsEval = 11;    // count, dist2, y^2 + z^2, x^2 + z^2, x^2 + y^2, xy, xz, yz, x, y, z
// entry (i, j), i <= j, of the matrix from the reduced sums t; "+ 0.0" keeps a negated zero sum from showing as -0
__device__ __forceinline__ double icp_info_entry(const double* t, int i, int j)
{
  switch (i * 6 + j) {
    case 0: return t[2];  case 1: return -t[5] + 0.0;  case 2: return -t[6] + 0.0;  case 4: return -t[10] + 0.0;  case 5: return t[9];
    case 7: return t[3];  case 8: return -t[7] + 0.0;  case 9: return t[10];  case 11: return -t[8] + 0.0;
    case 14: return t[4];  case 15: return -t[9] + 0.0;  case 16: return t[8];
    case 21: case 28: case 35: return t[0];
    default: return 0.0;
  }
}

// path record of a quad (tr_paths): bits 2 s, 2 s + 1 = what lane s did with its slice of the LDS-resident targets, bit 8 = the winner came from the tail
constexpr int kIcpPathNone = 0, kIcpPathSingle = 1, kIcpPathWalk = 2, kIcpPathTailWon = 256;

template <int N>
__device__ __forceinline__ void block_reduce(double (&v)[N], double* red /*[waves][N]*/, double* tot /*[N]*/)
{
#pragma unroll
  for (int k = 0; k < N; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < N; ++k) red[(threadIdx.x >> 6) * N + k] = v[k];
  __syncthreads();
  if (threadIdx.x < N) {
    double s = 0.0;
    for (int w = 0; w < kIcpThreads / 64; ++w) s += red[w * N + threadIdx.x];   // fixed order: deterministic
    tot[threadIdx.x] = s;
  }
  __syncthreads();
}

// pair b of a launch: where its source and its target start in the blobs, and their sizes (a kernel that reads one cloud takes those fields alone).
// Used where it leaves the kernel's instructions as they were: the loop kernel of the two surface estimates and the two grid builds
struct IcpPair { long long s_lo, n1, t_lo, n2; };
__device__ __forceinline__ IcpPair icp_pair(const IcpArgs& a, int b)
{
  const long long row = a.rows ? a.rows[b] : b;
  IcpPair p;
  p.s_lo = a.off[row * 2]; p.n1 = a.off[(row + 1) * 2] - p.s_lo;
  p.t_lo = a.off[row * 2 + 1]; p.n2 = a.off[(row + 1) * 2 + 1] - p.t_lo;
  return p;
}

// kTrace: the SAME scan, and behind the quad's merge one record per source point (IcpArgs::tr_*) -- the test hook's instantiations; the
// shipped ones (kTrace = false) compile to what they were without it (per-kernel resource remarks unchanged)
// kGrid: the grid search in place of the scan (one lane per source point, the bucket table in LDS); loop, sums, estimate and stop are the same source
// kEval: the evaluation call (IcpEvalArgs): the same search, the sums above in place of the estimate's, out after the first evaluation, no transform
// written.  The other instantiations compile to what they were without it (DESIGN.md 4.7f has the remarks of both)
template <bool kFull, bool kTrace = false, bool kGrid = false, bool kEval = false>
__global__ __launch_bounds__(kIcpThreads) void icp_kernel(const std::conditional_t<kEval, IcpEvalArgs, std::conditional_t<kGrid, IcpGridArgs, IcpArgs>> a)
{
  static_assert(!kEval || (!kFull && !kTrace), "the evaluation has no estimate and no trace");
  constexpr int kSplit = kGrid ? 1 : kIcpSplit;   // lanes per source point
  constexpr int kSums = kEval ? kIcpSumsEval : kFull ? kIcpSumsFull : kIcpSums;
  extern __shared__ __attribute__((aligned(16))) double tgt[];   // [3][lds_points] doubles | [3][4 slices][S4] floats
  __shared__ double T[12];            // rows 0..2 of the 4x4
  __shared__ double red[(kIcpThreads / 64) * kSums], tot[kSums];
  const int b = blockIdx.x, tid = threadIdx.x, sub = tid & (kSplit - 1);
  const long long row = a.rows ? a.rows[b] : b;
  const long long s_lo = a.off[row * 2], n1 = a.off[(row + 1) * 2] - s_lo;
  const long long t_lo = a.off[row * 2 + 1], n2 = a.off[(row + 1) * 2 + 1] - t_lo;
  const float* src = a.pts[0] + s_lo * 3;
  const float* dst = a.pts[1] + t_lo * 3;
  if (tid < 12) T[tid] = a.init[(size_t)b * 16 + tid];
  const int nl = (int)min((long long)a.lds_points, n2);
  const double* tx = tgt; const double* ty = tgt + a.lds_points; const double* tz = tgt + 2 * a.lds_points;
  const int S4 = icp_slice_len(a.lds_points);
  float* t32 = reinterpret_cast<float*>(tgt + 3 * (size_t)a.lds_points);   // [coordinate][slice][S4]
  // grid search: the pair's grid, its bucket starts copied to LDS (the records stay in L2)
  [[maybe_unused]] IcpGridView g = {};
  if constexpr (kGrid) {
    g = icp_grid_view(a.ws + a.ws_off[b], n2);
    int* const lds = reinterpret_cast<int*>(tgt);
    for (int j = tid; j <= g.buckets; j += kIcpThreads) lds[j] = g.start[j];
    g.start = lds;   // the search reads the LDS copy
  } else {
  for (int j = tid; j < 3 * kIcpSplit * S4; j += kIcpThreads) t32[j] = kIcpFar;
  __syncthreads();
  for (int j = tid; j < nl; j += kIcpThreads) {
    const float x = dst[j * 3], y = dst[j * 3 + 1], z = dst[j * 3 + 2];
    tgt[j] = (double)x; tgt[a.lds_points + j] = (double)y; tgt[2 * a.lds_points + j] = (double)z;
    const int o = (j & (kIcpSplit - 1)) * S4 + (j >> 2);
    t32[o] = x; t32[kIcpSplit * S4 + o] = y; t32[2 * kIcpSplit * S4 + o] = z;
  }
  }
  __syncthreads();
  const int Lp = ((nl + kIcpSplit - 1) / kIcpSplit + 1) & ~1;   // slice positions walked (even; the padding behind a slice's end is kIcpFar)
  const float* s32x = t32 + sub * S4; const float* s32y = s32x + kIcpSplit * S4; const float* s32z = s32y + kIcpSplit * S4;
  const double r2 = a.radius * a.radius;
  // the correspondence sums are taken about a pivot near the clouds (the first target point), not about the origin: one-pass centring
  // sum p q - n mean(p) mean(q) cancels |offset|^2 / extent^2 of its digits (a cloud 4 km from the origin: the rotation came out 6e-8 off
  // Open3D's two-pass estimate, tests/test_icp_gpu.py::test_icp_exact_ties_and_far_frames); about the pivot the terms are of the clouds' size
  const double cx = n2 > 0 ? (double)dst[0] : 0.0, cy = n2 > 0 ? (double)dst[1] : 0.0, cz = n2 > 0 ? (double)dst[2] : 0.0;
  [[maybe_unused]] double ex = 0.0, ey = 0.0, ez = 0.0;   // kEval: the centre of the information matrix (the caller's, or the origin)
  if constexpr (kEval)
    if (a.centers) { ex = a.centers[(size_t)b * 3]; ey = a.centers[(size_t)b * 3 + 1]; ez = a.centers[(size_t)b * 3 + 2]; }
  double fit_prev = 0.0, rmse_prev = 0.0, fit = 0.0, rmse = 0.0;
  int k = 0;
  if (n1 > 0 && n2 > 0)
    for (k = 0;; ++k) {
      // ---- evaluate(T): nearest target point of every transformed source point, sums over the inliers ----
      double v[kSums];
#pragma unroll
      for (int q = 0; q < kSums; ++q) v[q] = 0.0;
      for (long long i0 = 0; i0 < n1; i0 += kIcpThreads / kSplit) {
        const long long i = i0 + (tid / kSplit);
        const bool active = i < n1;                      // (inactive quads run along on the last point: the shuffles below want every lane)
        const long long ic = active ? i : n1 - 1;
        const double sx = src[ic * 3], sy = src[ic * 3 + 1], sz = src[ic * 3 + 2];
        const double px = T[0] * sx + T[1] * sy + T[2] * sz + T[3];
        const double py = T[4] * sx + T[5] * sy + T[6] * sz + T[7];
        const double pz = T[8] * sx + T[9] * sy + T[10] * sz + T[11];
        double best = 1e300; int bj = 0x7fffffff;
        int path = kIcpPathNone;
        [[maybe_unused]] float4 brec = {0.f, 0.f, 0.f, 0.f};   // grid search: the winner's record
        if constexpr (kGrid) {
          if (active) icp_grid_nearest<kTrace>(px, py, pz, g, best, bj, brec, path);
        } else {
        {
          // one fp32 pass over the slice: its smallest distance m1 with the position it sits at, and its second smallest m2 (v_med3 of the
          // ordered pair and the newcomer) -- four vector instructions per target next to the packed arithmetic, no branch
          const float pxf = (float)px, pyf = (float)py, pzf = (float)pz;
          const icp_f32x2 qx2 = {pxf, pxf}, qy2 = {pyf, pyf}, qz2 = {pzf, pzf};
          float m1 = 3.0e38f, m2 = 3.0e38f;
          int im = 0;
#pragma unroll 4
          for (int m = 0; m < Lp; m += 2) {
            const icp_f32x2 X = *reinterpret_cast<const icp_f32x2*>(s32x + m), Y = *reinterpret_cast<const icp_f32x2*>(s32y + m), Z = *reinterpret_cast<const icp_f32x2*>(s32z + m);
            const icp_f32x2 dx = qx2 - X, dy = qy2 - Y, dz = qz2 - Z;
            const icp_f32x2 e = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
#pragma unroll
            for (int u = 0; u < 2; ++u) {
              const bool lt = e[u] < m1;
              m2 = __builtin_amdgcn_fmed3f(m1, m2, e[u]);   // m1 <= m2: the median of the three is the new second smallest
              im = lt ? m + u : im;
              m1 = fminf(m1, e[u]);
            }
          }
          float qm = fminf(m1, __shfl_xor(m1, 1));
          qm = fminf(qm, __shfl_xor(qm, 2));
          const float P = fabsf(pxf) + fabsf(pyf) + fabsf(pzf) + 1e-30f;
          const float thr = qm + 4.f * icp_prefilter_eps(P, 1.01f * qm + 1e-6f * P * P);
          // every target whose fp64 distance is the minimum has an fp32 distance <= thr.  A lane with ONE such target decides it in fp64; a lane
          // with two or more (a near-tie inside its slice: rare) walks its slice in fp64 as the all-fp64 kernel did
          if (m2 <= thr) {
            if constexpr (kTrace) path = kIcpPathWalk;
#pragma unroll 1
            for (int j = sub; j < nl; j += kIcpSplit) {
              const double ddx = px - tx[j], ddy = py - ty[j], ddz = pz - tz[j];
              const double d = ddx * ddx + ddy * ddy + ddz * ddz;
              if (d < best) { best = d; bj = j; }   // strict: the first index of this lane's slice wins ties
            }
          } else if (m1 <= thr) {
            if constexpr (kTrace) path = kIcpPathSingle;
            const int j = sub + kIcpSplit * im;
            if (j < nl) {
              const double ddx = px - tx[j], ddy = py - ty[j], ddz = pz - tz[j];
              best = ddx * ddx + ddy * ddy + ddz * ddz; bj = j;
            }
          }
        }
#pragma unroll 1
        for (long long j = nl + sub; j < n2; j += kIcpSplit) {   // clouds larger than the LDS budget: the tail comes from L2
          const double dx = px - (double)dst[j * 3], dy = py - (double)dst[j * 3 + 1], dz = pz - (double)dst[j * 3 + 2];
          const double d = dx * dx + dy * dy + dz * dz;
          if (d < best) { best = d; bj = (int)j; }
        }
        // the quad's minimum; equal distances go to the lower index (oracle: argmin = the first index)
#pragma unroll
        for (int o = 1; o < kIcpSplit; o <<= 1) {
          const double ob = __shfl_xor(best, o);
          const int oj = __shfl_xor(bj, o);
          if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
        }
        }
        if constexpr (kTrace && kGrid) {
          if (active && k == 0) {
            const bool found = bj != 0x7fffffff;
            a.tr_index[i] = found ? bj : -1; a.tr_dist[i] = found ? best : __builtin_huge_val(); a.tr_inlier[i] = best <= r2; a.tr_paths[i] = path;
          }
        }
        if constexpr (kTrace && !kGrid) {
          path <<= 2 * sub;
          path |= __shfl_xor(path, 1);
          path |= __shfl_xor(path, 2);
          if (active && sub == 0 && k == 0) {
            a.tr_index[i] = bj; a.tr_dist[i] = best; a.tr_inlier[i] = best <= r2;
            a.tr_paths[i] = path | (bj >= nl ? kIcpPathTailWon : 0);
          }
        }
        if constexpr (kEval) {
          if (active && sub == 0) {
            const bool in = best <= r2;
            if (a.corr) a.corr[a.corr_off[b] + i] = in ? bj : -1;
            if (in) {
              v[0] += 1.0; v[1] += best;
              if (a.info) {
                const double x = (kGrid ? (double)brec.x : bj < nl ? tx[bj] : (double)dst[(long long)bj * 3]) - ex;
                const double y = (kGrid ? (double)brec.y : bj < nl ? ty[bj] : (double)dst[(long long)bj * 3 + 1]) - ey;
                const double z = (kGrid ? (double)brec.z : bj < nl ? tz[bj] : (double)dst[(long long)bj * 3 + 2]) - ez;
                v[2] += y * y + z * z; v[3] += x * x + z * z; v[4] += x * x + y * y;
                v[5] += x * y; v[6] += x * z; v[7] += y * z; v[8] += x; v[9] += y; v[10] += z;
              }
            }
          }
        } else
        if (active && sub == 0 && best <= r2) {
          const double qx = kGrid ? (double)brec.x : bj < nl ? tx[bj] : (double)dst[(long long)bj * 3];
          const double qy = kGrid ? (double)brec.y : bj < nl ? ty[bj] : (double)dst[(long long)bj * 3 + 1];
          const double qz = kGrid ? (double)brec.z : bj < nl ? tz[bj] : (double)dst[(long long)bj * 3 + 2];
          const double ax = px - cx, ay = py - cy, az = pz - cz, bx = qx - cx, by = qy - cy, bz = qz - cz;
          v[0] += 1.0; v[1] += ax; v[2] += ay; v[3] += az; v[4] += bx; v[5] += by; v[6] += bz;
          if constexpr (kFull) {   // sum b a^T, row-major
            v[7] += bx * ax; v[8] += bx * ay; v[9] += bx * az;
            v[10] += by * ax; v[11] += by * ay; v[12] += by * az;
            v[13] += bz * ax; v[14] += bz * ay; v[15] += bz * az; v[16] += best;
            v[17] += ax * ax + ay * ay + az * az; v[18] += bx * bx + by * by + bz * bz;
          } else {
            v[7] += ax * bx + ay * by; v[8] += ax * by - ay * bx; v[9] += best;
            v[10] += ax * ax + ay * ay; v[11] += bx * bx + by * by;
          }
        }
      }
      block_reduce(v, red, tot);
      const double cnt = tot[0];
      fit = cnt / (double)n1;
      rmse = cnt > 0.0 ? sqrt(tot[kEval ? 1 : kFull ? 16 : 9] / cnt) : 0.0;
      if constexpr (kEval) break;   // one evaluation: the exit of its = 0
      if (k > 0 && fabs(fit - fit_prev) < 1e-6 && fabs(rmse - rmse_prev) < 1e-6) break;
      if (k == a.its) break;
      fit_prev = fit; rmse_prev = rmse;
      if constexpr (kFull) {
        // ---- estimate: rotation + translation minimising sum |R p + t - q|^2 over the correspondences (Umeyama, no scaling) ----
        if (tid == 0 && cnt > 0.0) {
          const double am[3] = {tot[1] / cnt, tot[2] / cnt, tot[3] / cnt}, bm[3] = {tot[4] / cnt, tot[5] / cnt, tot[6] / cnt};   // about the pivot
          double* const Rm = red + 18;   // (red is free until the next block_reduce: A, the SVD's work, R)
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) red[i * 3 + j] = tot[7 + i * 3 + j] - cnt * (bm[i] * am[j]);
          double fro = 0.0;
#pragma unroll
          for (int i = 0; i < 9; ++i) fro += red[i] * red[i];
          const double noise = kIcpNoise * cnt * sqrt(tot[17] * tot[18]);
          if (fro > noise * noise)
            icp_umeyama_rotation(red);
          else
            for (int i = 0; i < 9; ++i) Rm[i] = i % 4 == 0 ? 1.0 : 0.0;   // no rotation is determined: keep it
          const double mp[3] = {cx + am[0], cy + am[1], cz + am[2]}, mq[3] = {cx + bm[0], cy + bm[1], cz + bm[2]};
          // T <- U T,  U = [R | mean q - R mean p]
          double n[12];
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            for (int col = 0; col < 4; ++col) n[r * 4 + col] = Rm[r * 3] * T[col] + Rm[r * 3 + 1] * T[4 + col] + Rm[r * 3 + 2] * T[8 + col];
            n[r * 4 + 3] += mq[r] - (Rm[r * 3] * mp[0] + Rm[r * 3 + 1] * mp[1] + Rm[r * 3 + 2] * mp[2]);
          }
          for (int q = 0; q < 12; ++q) T[q] = n[q];
        }
      } else
      // ---- estimate: rotation about z + translation minimising sum |Rz p + t - q|^2 over the correspondences ----
      if (tid == 0 && cnt > 0.0) {
        const double apx = tot[1] / cnt, apy = tot[2] / cnt, apz = tot[3] / cnt;   // means about the pivot
        const double aqx = tot[4] / cnt, aqy = tot[5] / cnt, aqz = tot[6] / cnt;
        const double sxx = tot[7] - cnt * (apx * aqx + apy * aqy);
        const double sxy = tot[8] - cnt * (apx * aqy - apy * aqx);
        const double noise = kIcpNoise * cnt * sqrt(tot[10] * tot[11]);
        const double th = sxx * sxx + sxy * sxy > noise * noise ? atan2(sxy, sxx) : 0.0, c = cos(th), s = sin(th);   // (no rotation determined: keep it)
        const double mpx = cx + apx, mpy = cy + apy, mqx = cx + aqx, mqy = cy + aqy;
        const double tx = mqx - (c * mpx - s * mpy), ty = mqy - (s * mpx + c * mpy), tz = aqz - apz;
        // T <- U T,  U = [[c,-s,0,tx],[s,c,0,ty],[0,0,1,tz]]
        double n[12];
        for (int col = 0; col < 4; ++col) {
          n[col] = c * T[col] - s * T[4 + col];
          n[4 + col] = s * T[col] + c * T[4 + col];
          n[8 + col] = T[8 + col];
        }
        n[3] += tx; n[7] += ty; n[11] += tz;
        for (int q = 0; q < 12; ++q) T[q] = n[q];
      }
      __syncthreads();
    }
  __syncthreads();
  if constexpr (kEval) {
    // the 6x6 matrix from the reduced sums, the lower half mirrored; an empty cloud (no evaluation ran, tot is unset) gives the zero matrix
    if (a.info && tid < 36) {
      const int r = tid / 6, c = tid % 6;
      a.info[(size_t)b * 36 + tid] = n1 > 0 && n2 > 0 ? icp_info_entry(tot, min(r, c), max(r, c)) : 0.0;
    }
  } else {
  if (tid < 12) a.out[(size_t)b * 16 + tid] = T[tid];
  if (tid >= 12 && tid < 16) a.out[(size_t)b * 16 + tid] = tid == 15 ? 1.0 : 0.0;
  }
  if (tid == 0) {
    if (a.fitness) a.fitness[b] = fit;
    if (a.rmse) a.rmse[b] = rmse;
    if (a.iters) a.iters[b] = k;
  }
}

// Grid build, one workgroup per pair: cell edge from the pair's largest |coordinate|, then a counting sort of the targets by hashed cell -- counts by
// LDS atomics, an exclusive scan over the H buckets (each thread a contiguous run, the runs' totals scanned across the block), the starts written
// out, the scatter by LDS atomics on the running starts.  Both passes hash the same values, so the positions handed out stay inside [0, n2).
// The cloud is the caller's: `dst` [n2][3], its grid at `ws`, cells for `radius` (the kernels below name the target; the generalized estimate also
// grids the source)
__device__ __forceinline__ void icp_grid_build_cloud(const float* dst, long long n2, char* ws, double radius)
{
  extern __shared__ int cnt[];        // [H + 1]
  __shared__ double wmax[kIcpThreads / 64];
  __shared__ int wsum[kIcpThreads / 64], wocc[kIcpThreads / 64], wbig[kIcpThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const IcpGridView g = icp_grid_view(ws, n2, false);   // (its edge is found here)
  const int H = g.buckets;
  double m = 0.0;
  for (long long j = tid; j < n2; j += kIcpThreads)
    m = fmax(m, (double)fmaxf(fmaxf(fabsf(dst[j * 3]), fabsf(dst[j * 3 + 1])), fabsf(dst[j * 3 + 2])));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
  if (lane == 0) wmax[wave] = m;
  for (int j = tid; j <= H; j += kIcpThreads) cnt[j] = 0;
  __syncthreads();
  for (int q = 0; q < kIcpThreads / 64; ++q) m = fmax(m, wmax[q]);
  const double e = fmax(radius * (1.0 + kGridSpan), (m + radius) * kGridSpan);
  for (long long j = tid; j < n2; j += kIcpThreads)
    atomicAdd(&cnt[icp_grid_bucket((double)dst[j * 3], (double)dst[j * 3 + 1], (double)dst[j * 3 + 2], e, g.mask)], 1);
  __syncthreads();
  // exclusive scan: thread t owns buckets [t per, (t + 1) per)
  const int per = (H + kIcpThreads - 1) / kIcpThreads, lo = min(tid * per, H), hi = min(lo + per, H);
  int sum = 0, occ = 0, big = 0;
  for (int q = lo; q < hi; ++q) { const int c = cnt[q]; sum += c; occ += c > 0; big = max(big, c); }
  int inc = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(inc, o); if (lane >= o) inc += up; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { occ += __shfl_xor(occ, o); big = max(big, __shfl_xor(big, o)); }
  if (lane == 63) wsum[wave] = inc;
  if (lane == 0) { wocc[wave] = occ; wbig[wave] = big; }
  __syncthreads();
  int run = inc - sum;
  for (int q = 0; q < wave; ++q) run += wsum[q];
  __syncthreads();
  for (int q = lo; q < hi; ++q) { const int c = cnt[q]; cnt[q] = run; run += c; }
  if (tid == 0) {
    cnt[H] = (int)n2;
    int o2 = 0, b2 = 0;
    for (int q = 0; q < kIcpThreads / 64; ++q) { o2 += wocc[q]; b2 = max(b2, wbig[q]); }
    IcpGridInfo* info = reinterpret_cast<IcpGridInfo*>(g.ws);
    info->edge = e; info->buckets = H; info->occupied = o2; info->largest = b2; info->pad = 0;
  }
  __syncthreads();
  for (int j = tid; j <= H; j += kIcpThreads) g.start[j] = cnt[j];
  __syncthreads();
  for (long long j = tid; j < n2; j += kIcpThreads) {
    const float x = dst[j * 3], y = dst[j * 3 + 1], z = dst[j * 3 + 2];
    const int pos = atomicAdd(&cnt[icp_grid_bucket((double)x, (double)y, (double)z, e, g.mask)], 1);
    g.rec[pos] = make_float4(x, y, z, __int_as_float((int)j));
  }
}

__global__ __launch_bounds__(kIcpThreads) void icp_grid_build_kernel(const IcpGridArgs a)
{
  const int b = blockIdx.x;
  const IcpPair pr = icp_pair(a, b);
  icp_grid_build_cloud(a.pts[1] + pr.t_lo * 3, pr.n2, a.ws + a.ws_off[b], a.radius);
}

// shared driver: tables already on the device
// alignnet_debug_icp_scan: host arrays [n1] for the records of pair 0's first evaluation; lds_points > 0 overrides the LDS stage's size (<= the budget)
// alignnet_debug_icp_grid (grid = true): the same through the grid search, paths = candidates evaluated, info = pair 0's IcpGridInfo
struct IcpTraceOut { long long n1; int lds_points; int* index; double* dist; int* inlier; int* paths; int* lds_points_used; bool grid; IcpGridInfo* info; };

constexpr long long kIcpLdsBudget = (150 * 1024) / 36;   // doubles x 3 + floats x 3 per point within one CU's LDS
constexpr long long kIcpGridAuto = kIcpLdsBudget;        // "icp_search" = 2: pairs with n2 above this take the grid (where the scan leaves its certified LDS path)

template <class Args>
Args icp_args_from(const Args& a, int lo)   // the arguments of pairs lo.. as a launch of their own
{
  Args r = a;
  r.init += (size_t)lo * 16; r.out += (size_t)lo * 16; r.fitness += lo; r.rmse += lo; r.iters += lo;
  if (r.rows) r.rows += lo; else r.off += (size_t)lo * 2;
  return r;
}

// the clouds of a call as the kernels address them, with whatever this call uploaded of them (the dataset's tables stay the handle's)
struct IcpClouds {
  const float* pts[2] = {nullptr, nullptr}; const long long* off = nullptr; const int* rows = nullptr;
  std::vector<long long> n2;   // the target sizes of the B pairs as the host knows them
  std::vector<long long> n1;   // the source sizes (the generalized estimate carves a source grid per pair)
  PairUpload up; DevBuf<int> up_rows;
};

// clouds passed from the host (alignnet_icp_refine / _register / _plane_register and the read-backs); `name` is the entry point's in the messages
int stage_host(alignnet_handle* h, const std::string& name, const float* points1, const float* points2, const int64_t* offsets, int32_t B, IcpClouds* c)
{
  if (!h) return 1;
  if (upload_pairs(h, name, points1, points2, offsets, B, &c->up)) return 1;
  c->n2.swap(c->up.n2); c->n1.swap(c->up.n1);
  c->pts[0] = c->up.pts[0].p; c->pts[1] = c->up.pts[1].p; c->off = c->up.off.p;
  return 0;
}

// clouds of the uploaded dataset addressed by rows (the _dataset entry points)
int stage_rows(alignnet_handle* h, const std::string& name, const int32_t* rows, int32_t B, IcpClouds* c)
{
  if (!h) return 1;
  alignnet::DatasetTables t;
  if (!alignnet_dataset_tables(h, &t)) return fail(h, name + ": no dataset uploaded");
  if (!rows || B < 1) return fail(h, name + ": null rows or B < 1");
  for (int i = 0; i < B; ++i)
    if (rows[i] < 0 || rows[i] >= t.n) return fail(h, name + ": row " + std::to_string(rows[i]) + " out of range");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  HIP_TRY(h, c->up_rows.alloc((size_t)B));
  HIP_TRY(h, hipMemcpyAsync(c->up_rows.p, rows, (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  // target sizes from the host's copy of the offsets (the grid search carves its workspace per pair)
  c->n2.resize(B); c->n1.resize(B);
  for (int i = 0; i < B; ++i) {
    c->n2[i] = t.h_off[((size_t)rows[i] + 1) * 2 + 1] - t.h_off[(size_t)rows[i] * 2 + 1];
    c->n1[i] = t.h_off[((size_t)rows[i] + 1) * 2] - t.h_off[(size_t)rows[i] * 2];
  }
  c->pts[0] = t.pts[0]; c->pts[1] = t.pts[1]; c->off = t.off; c->rows = c->up_rows.p;
  return 0;
}

// the results of a call on the device: `init` goes up when the arguments are bound, what the caller asked for comes down at the end
struct IcpResults {
  DevBuf<double> init, out, fr; DevBuf<int> it;   // fr: fitness [B] | rmse [B]
  int up(alignnet_handle* h, int B, const double* host_init, IcpArgs* a)
  {
    HIP_TRY(h, init.alloc((size_t)B * 16));
    HIP_TRY(h, out.alloc((size_t)B * 16));
    HIP_TRY(h, fr.alloc((size_t)B * 2));
    HIP_TRY(h, it.alloc((size_t)B));
    HIP_TRY(h, hipMemcpyAsync(init.p, host_init, (size_t)B * 16 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    a->init = init.p; a->out = out.p; a->fitness = fr.p; a->rmse = fr.p + B; a->iters = it.p;
    return 0;
  }
  int down(alignnet_handle* h, int B, double* host_out, double* fitness, double* rmse, int* iters)   // ends with the call's one synchronisation
  {
    HIP_TRY(h, hipMemcpyAsync(host_out, out.p, (size_t)B * 16 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (fitness) HIP_TRY(h, hipMemcpyAsync(fitness, fr.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (rmse) HIP_TRY(h, hipMemcpyAsync(rmse, fr.p + B, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (iters) HIP_TRY(h, hipMemcpyAsync(iters, it.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return 0;
  }
};

// the handle's workspace, grown to `need` bytes (the chunks of a call carve it in stream order)
int reserve_grid_ws(alignnet_handle* h, size_t need)
{
  if (grow_bytes(h, &h->icp_grid_ws, &h->icp_grid_ws_bytes, need)) return 1;
  h->icp_grid_ws_used = need;
  return 0;
}

// which search each pair takes under `mode` (the "icp_search" values), and the grid pairs' workspace: consecutive grid pairs form chunks of at most
// kIcpGridWsBudget (one pair may exceed it alone; a chunk's first pair sits at offset 0), every chunk reuses the handle's workspace in stream order.
// need: the bytes reserved, 0 when no pair takes the grid
int plan_search(alignnet_handle* h, int mode, const std::vector<long long>& n2, std::vector<char>* grid, std::vector<long long>* ws_off, size_t* need)
{
  const int B = (int)n2.size();
  grid->assign(B, 0);
  ws_off->assign(B, 0);
  size_t cur = 0; int open = -1;
  *need = 0;
  for (int b = 0; b < B; ++b) {
    (*grid)[b] = mode == 1 || (mode == 2 && n2[b] > kIcpGridAuto);
    if (!(*grid)[b]) { open = -1; continue; }
    if (n2[b] > 0x7fffffff) return fail(h, "icp: more than 2^31 - 1 target points in a pair");
    const size_t bytes = icp_grid_pair_bytes(n2[b]);
    if (open < 0 || cur + bytes > kIcpGridWsBudget) { open = b; cur = 0; }
    (*ws_off)[b] = (long long)cur; cur += bytes;
    *need = std::max(*need, cur);
  }
  if (*need && reserve_grid_ws(h, *need)) return 1;
  return 0;
}

// the launches over plan_search's result, in order: pairs [lo, hi) are a run of scan pairs or one chunk of grid pairs (a chunk's first pair sits at
// offset 0); big: the chunk's largest target; lds: the dynamic LDS of the run's kernels.  Starts from {0, 0}
struct IcpRun { int lo, hi; bool grid; long long big; size_t lds; };
bool next_run(const std::vector<char>& grid, const std::vector<long long>& ws_off, const std::vector<long long>& n2, int lds_points, IcpRun* r)
{
  const int B = (int)grid.size();
  r->lo = r->hi;
  if (r->lo >= B) return false;
  r->hi = r->lo + 1; r->grid = grid[r->lo]; r->big = n2[r->lo];
  if (!r->grid) {
    while (r->hi < B && !grid[r->hi]) ++r->hi;
    r->lds = icp_lds_bytes(lds_points);
  } else {
    while (r->hi < B && grid[r->hi] && ws_off[r->hi] != 0) { r->big = std::max(r->big, n2[r->hi]); ++r->hi; }
    r->lds = ((size_t)icp_grid_buckets(r->big) + 1) * 4;
  }
  return true;
}

// the grids of a chunk's targets (the build reads the clouds, the radius and the workspace)
void launch_grid_build(alignnet_handle* h, const IcpGridArgs& g, const IcpRun& r)
{
  alignnet::ProfScope prof_scope(h, alignnet::PK_ICP_GRID_BUILD);
  hipLaunchKernelGGL(icp_grid_build_kernel, dim3(r.hi - r.lo), dim3(kIcpThreads), r.lds, h->stream, g);
}

// the loop kernels by argument type: one entry serves the attribute call and the launch
using Scan = void (*)(const IcpArgs);
using Grid = void (*)(const IcpGridArgs);
using Eval = void (*)(const IcpEvalArgs);
constexpr Scan kIcpScan[2][2] = {{icp_kernel<false>, icp_kernel<true>}, {icp_kernel<false, true>, icp_kernel<true, true>}};   // [trace][full]
constexpr Grid kIcpGrid[2][2] = {{icp_kernel<false, false, true>, icp_kernel<true, false, true>}, {icp_kernel<false, true, true>, icp_kernel<true, true, true>}};
constexpr Eval kIcpEval[2] = {icp_kernel<false, false, false, true>, icp_kernel<false, false, true, true>};   // [grid]

// a kernel's dynamic-LDS ceiling, raised once per device
template <class Kernel>
int raise_lds(alignnet_handle* h, alignnet::PerDeviceOnce* once, Kernel kernel)
{
  if (!once->need(h->cfg.device)) return 0;
  HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096));
  once->mark(h->cfg.device);
  return 0;
}

// stage_n2: what the scan's LDS stage is sized for
int run_icp(alignnet_handle* h, const IcpClouds& c, long long stage_n2, int B, const double* init, double radius, int its, bool full, double* out,
            double* fitness, double* rmse, int* iters, const IcpTraceOut* trace = nullptr, const alignnet::IcpDeviceIo* dev = nullptr)
{
  // dev: init / out / fitness / rmse / iters are device buffers of the caller (alignnet_icp_run_device): nothing is allocated, uploaded, downloaded
  // or waited for here -- the launches are the same
  const std::vector<long long>& n2 = c.n2;
  if (!init || !out) return fail(h, "icp: null init / out");
  if (!(radius > 0.0) || its < 0) return fail(h, "icp: radius must be > 0 and its >= 0");
  // which search each pair takes ("icp_search"; the read-backs choose their own), and the grid pairs' workspace: consecutive grid pairs form
  // chunks of at most kIcpGridWsBudget (one pair may exceed it alone), every chunk reuses the handle's workspace in stream order
  const int mode = trace ? (trace->grid ? 1 : 0) : h->icp_search;
  std::vector<char> grid;
  std::vector<long long> ws_off_own;
  std::vector<long long>& ws_off = dev ? *dev->h_ws_off : ws_off_own;
  size_t need = 0;
  if (plan_search(h, mode, n2, &grid, &ws_off, &need)) return 1;
  IcpGridArgs a;
  IcpResults res;
  DevBuf<long long> wsoff;
  if (dev) { a.init = init; a.out = out; a.fitness = fitness; a.rmse = rmse; a.iters = iters; }
  else if (res.up(h, B, init, &a)) return 1;
  long long* const d_ws_off = dev ? dev->ws_off : nullptr;
  if (need) {
    if (!dev) HIP_TRY(h, wsoff.alloc((size_t)B));
    HIP_TRY(h, hipMemcpyAsync(dev ? d_ws_off : wsoff.p, ws_off.data(), (size_t)B * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  }
  a.pts[0] = c.pts[0]; a.pts[1] = c.pts[1]; a.off = c.off; a.rows = c.rows; a.radius = radius; a.its = its;
  a.lds_points = (int)std::max<long long>(1, std::min(kIcpLdsBudget, stage_n2));
  a.tr_index = a.tr_inlier = a.tr_paths = nullptr; a.tr_dist = nullptr;
  a.ws = static_cast<char*>(h->icp_grid_ws); a.ws_off = dev ? d_ws_off : wsoff.p;
  DevBuf<char> tr;   // [n1] doubles | 3 x [n1] ints
  if (trace) {
    if (trace->lds_points > 0) a.lds_points = trace->lds_points;
    const size_t n = (size_t)std::max<long long>(trace->n1, 1);
    HIP_TRY(h, tr.alloc(n * 20));
    HIP_TRY(h, hipMemsetAsync(tr.p, 0xff, n * 20, h->stream));   // (index -1 where the kernel wrote nothing: an empty target)
    a.tr_dist = reinterpret_cast<double*>(tr.p);
    a.tr_index = reinterpret_cast<int*>(tr.p + n * 8); a.tr_inlier = a.tr_index + n; a.tr_paths = a.tr_inlier + n;
  }
  static alignnet::PerDeviceOnce attr[9];   // [which]: scan, [which + 4]: grid, [8]: the build
  const int which = (full ? 1 : 0) + (trace ? 2 : 0);
  const Scan scan = kIcpScan[trace != nullptr][full];
  const Grid search = kIcpGrid[trace != nullptr][full];
  if (raise_lds(h, &attr[which], scan)) return 1;
  if (need && (raise_lds(h, &attr[which + 4], search) || raise_lds(h, &attr[8], icp_grid_build_kernel))) return 1;
  for (IcpRun run = {0, 0}; next_run(grid, ws_off, n2, a.lds_points, &run);) {
    const dim3 pairs(run.hi - run.lo);
    if (!run.grid)
      hipLaunchKernelGGL(scan, pairs, dim3(kIcpThreads), run.lds, h->stream, icp_args_from<IcpArgs>(a, run.lo));
    else {
      IcpGridArgs r = icp_args_from<IcpGridArgs>(a, run.lo);
      r.ws_off += run.lo;
      launch_grid_build(h, r, run);
      alignnet::ProfScope prof_scope(h, alignnet::PK_ICP_GRID);
      hipLaunchKernelGGL(search, pairs, dim3(kIcpThreads), run.lds, h->stream, r);
    }
    HIP_TRY(h, hipGetLastError());
  }
  if (trace) {
    const size_t n = (size_t)std::max<long long>(trace->n1, 1), m = (size_t)trace->n1;
    if (m) {
      HIP_TRY(h, hipMemcpyAsync(trace->dist, tr.p, m * 8, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipMemcpyAsync(trace->index, tr.p + n * 8, m * 4, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipMemcpyAsync(trace->inlier, tr.p + n * 12, m * 4, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipMemcpyAsync(trace->paths, tr.p + n * 16, m * 4, hipMemcpyDeviceToHost, h->stream));
    }
    if (trace->grid) HIP_TRY(h, hipMemcpyAsync(trace->info, h->icp_grid_ws, sizeof(IcpGridInfo), hipMemcpyDeviceToHost, h->stream));
    else *trace->lds_points_used = a.lds_points;
  }
  if (dev) return 0;
  return res.down(h, B, out, fitness, rmse, iters);
}

// stage, then run: the point-to-point entry points on clouds from the host and on rows of the dataset; `fn` names the entry point in the messages
int icp_host(alignnet_handle* h, const char* fn, const float* points1, const float* points2, const int64_t* offsets, int32_t B, const double* init,
             double radius, int32_t its, bool full, double* out, double* fitness, double* rmse, int32_t* iterations, const IcpTraceOut* trace = nullptr)
{
  IcpClouds c;
  if (stage_host(h, fn, points1, points2, offsets, B, &c)) return 1;
  return run_icp(h, c, *std::max_element(c.n2.begin(), c.n2.end()), B, init, radius, its, full, out, fitness, rmse, iterations, trace);
}

int icp_rows(alignnet_handle* h, const char* fn, const int32_t* rows, int32_t B, const double* init, double radius, int32_t its, bool full,
             double* out, double* fitness, double* rmse, int32_t* iterations)
{
  IcpClouds c;
  if (stage_rows(h, fn, rows, B, &c)) return 1;
  // the scan's LDS stage stays sized for the budget whatever the rows hold, as it was when the host did not know the sizes: the kernel clamps per pair
  return run_icp(h, c, kIcpLdsBudget, B, init, radius, its, full, out, fitness, rmse, iterations);
}

// ---- evaluation of given transforms (alignnet_evaluate_registration*): icp_kernel<false, false, kGrid, true>, one launch per run of pairs -----------
// what the entry points check before anything is staged or queued
int eval_arguments(alignnet_handle* h, const std::string& fn, int32_t B, const double* transforms, double threshold, const double* fitness, const double* rmse)
{
  if (B < 1) return fail(h, fn + ": B < 1");
  if (!transforms || !fitness || !rmse) return fail(h, fn + ": null transforms / fitness / rmse");
  if (!(threshold > 0.0)) return fail(h, fn + ": threshold must be > 0");
  return 0;
}

// corr_off [B]: where pair b's source range starts in `correspondences`, corr_total its length.  The search per pair, the grid workspace and its chunks
// are run_icp's (plan_search); one synchronisation, at the end, with the downloads
int run_eval(alignnet_handle* h, const IcpClouds& c, long long stage_n2, int B, const double* transforms, double threshold, const double* centers,
             double* fitness, double* rmse, double* information, int32_t* correspondences, const std::vector<long long>& corr_off, long long corr_total)
{
  std::vector<char> grid;
  std::vector<long long> ws_off;
  size_t need = 0;
  if (plan_search(h, h->icp_search, c.n2, &grid, &ws_off, &need)) return 1;
  DevBuf<double> tf, fr, cen, info;
  DevBuf<long long> tab;   // corr_off [B] | ws_off [B]
  DevBuf<int> corr;
  HIP_TRY(h, tf.alloc((size_t)B * 16));
  HIP_TRY(h, fr.alloc((size_t)B * 2));
  HIP_TRY(h, tab.alloc((size_t)B * 2));
  HIP_TRY(h, hipMemcpyAsync(tf.p, transforms, (size_t)B * 16 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(tab.p, corr_off.data(), (size_t)B * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(tab.p + B, ws_off.data(), (size_t)B * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  if (centers) {
    HIP_TRY(h, cen.alloc((size_t)B * 3));
    HIP_TRY(h, hipMemcpyAsync(cen.p, centers, (size_t)B * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  if (information) HIP_TRY(h, info.alloc((size_t)B * 36));
  if (correspondences) {
    HIP_TRY(h, corr.alloc((size_t)std::max<long long>(corr_total, 1)));
    HIP_TRY(h, hipMemsetAsync(corr.p, 0xff, (size_t)std::max<long long>(corr_total, 1) * sizeof(int), h->stream));   // -1 where no evaluation runs (an empty target)
  }
  IcpEvalArgs a;
  a.pts[0] = c.pts[0]; a.pts[1] = c.pts[1]; a.off = c.off; a.rows = c.rows; a.init = tf.p; a.radius = threshold; a.its = 0;
  a.lds_points = (int)std::max<long long>(1, std::min(kIcpLdsBudget, stage_n2));
  a.out = nullptr; a.fitness = fr.p; a.rmse = fr.p + B; a.iters = nullptr;
  a.tr_index = a.tr_inlier = a.tr_paths = nullptr; a.tr_dist = nullptr;
  a.ws = static_cast<char*>(h->icp_grid_ws); a.ws_off = tab.p + B;
  a.centers = cen.p; a.info = info.p; a.corr = corr.p; a.corr_off = tab.p;
  static alignnet::PerDeviceOnce attr[3];   // scan, grid, the build
  if (raise_lds(h, &attr[0], kIcpEval[0])) return 1;
  if (need && (raise_lds(h, &attr[1], kIcpEval[1]) || raise_lds(h, &attr[2], icp_grid_build_kernel))) return 1;
  for (IcpRun run = {0, 0}; next_run(grid, ws_off, c.n2, a.lds_points, &run);) {
    const int lo = run.lo;
    IcpEvalArgs r = a;   // pairs lo.. as a launch of their own
    r.init += (size_t)lo * 16; r.fitness += lo; r.rmse += lo; r.corr_off += lo; r.ws_off += lo;
    if (r.centers) r.centers += (size_t)lo * 3;
    if (r.info) r.info += (size_t)lo * 36;
    if (r.rows) r.rows += lo; else r.off += (size_t)lo * 2;
    if (!run.grid)
      hipLaunchKernelGGL(kIcpEval[0], dim3(run.hi - lo), dim3(kIcpThreads), run.lds, h->stream, r);
    else {
      launch_grid_build(h, r, run);
      alignnet::ProfScope prof_scope(h, alignnet::PK_ICP_GRID);
      hipLaunchKernelGGL(kIcpEval[1], dim3(run.hi - lo), dim3(kIcpThreads), run.lds, h->stream, r);
    }
    HIP_TRY(h, hipGetLastError());
  }
  HIP_TRY(h, hipMemcpyAsync(fitness, fr.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(rmse, fr.p + B, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (information) HIP_TRY(h, hipMemcpyAsync(information, info.p, (size_t)B * 36 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (correspondences && corr_total) HIP_TRY(h, hipMemcpyAsync(correspondences, corr.p, (size_t)corr_total * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return 0;
}

// ---- point-to-plane ICP (alignnet_icp_plane_register*): target normals once per call, a 6x6 / 4x4 normal-equation estimate in the loop -------------
// Semantics: tests/icp_plane_ref.py (the reference names the method and leaves it `assert False`, icp.py:81-82).  Per pair, once per call: grid A
// (cells of `radius`) for the correspondence search and grid B (cells of `normal_radius`) for the normals, both by icp_grid_build_kernel; grid B's
// records are then put in original-index order inside every bucket (icp_plane_sort_kernel: the build's scatter orders them by its atomics, and the
// normals' fp64 moments would differ in their last bits from run to run); icp_plane_normals_kernel, one lane per target point over several workgroups
// per pair, takes count, first and second moments of the differences q_j - q_i over all targets with fp64 squared distance <= fl(normal_radius^2) (the
// point itself included, no cap on their number) and writes the unit eigenvector of the smallest eigenvalue of S2 / K - m m^T with n_z >= 0, or
// (0, 0, 1) for K < 3.  A bucket reached through two of the 27 cells is walked once: sums, unlike the minimum of the search, would count it twice.
// The cell claim of the grid search (file header) holds for a target as the query and normal_radius as the radius: same arithmetic, same bound.
// Loop (icp_surface_kernel<false, .>, one workgroup per pair, always the grid search): evaluate, stop test, estimate, T <- U T exactly as icp_kernel.  Estimate over
// the inlier correspondences (p, q, n): r = (p - q) . n, a = p - c (c = the pivot, the pair's first target), J = [a x n, n] (full) or [(a x n)_z, n]
// (z-constrained); J^T J x = -J^T r by Cholesky without pivoting on the diagonally scaled matrix; U = Tr(c) [Rz(g) Ry(b) Rx(a) | t] Tr(-c).  A diagonal
// entry <= 0, a pivot <= kIcpPlanePivot or no correspondence determines no update: U = I.
// The transformed point and the residual are evaluated WITHOUT fused multiply-adds, in the order the restatement states, so that both are the
// restatement's to the last bit at any distance from the origin (a cloud 5 km out: one fused product moves p by 1e-12 m and a residual of a millimetre
// by 1e-9 of itself); the squared distance is the grid search's expression.
constexpr int kIcpPlaneSums = 16, kIcpPlaneSumsFull = 29;   // count, sum d^2, upper triangle of J^T J (10 / 21), J^T r (4 / 6)
constexpr double kIcpPlanePivot = 1e-10;                    // on the scaled matrix (unit diagonal): a design constant
constexpr int kIcpPlaneLanes = 256, kIcpPlaneMaxBlocks = 1024;   // normals / sort: threads per workgroup, workgroups per pair at most

__host__ __device__ inline size_t icp_r256(size_t v) { return (v + 255) & ~(size_t)255; }
// a pair's workspace: grid A | grid B | grid B's records, index-ordered per bucket [n2] float4 | normals [n2][3] doubles | neighbour counts [n2] ints
__host__ __device__ inline size_t icp_plane_sorted_off(long long n2) { return 2 * icp_grid_pair_bytes(n2); }
__host__ __device__ inline size_t icp_plane_normals_off(long long n2) { return icp_plane_sorted_off(n2) + icp_r256((size_t)n2 * 16); }
__host__ __device__ inline size_t icp_plane_counts_off(long long n2) { return icp_plane_normals_off(n2) + icp_r256((size_t)n2 * 24); }
__host__ __device__ inline size_t icp_plane_pair_bytes(long long n2) { return icp_plane_counts_off(n2) + icp_r256((size_t)n2 * 4); }
// the three arrays behind the grids, from the view of the pair's grid A (the head of its part)
__device__ __forceinline__ float4* icp_plane_sorted(const IcpGridView& ga, long long n2) { return reinterpret_cast<float4*>(ga.ws + icp_plane_sorted_off(n2)); }
__device__ __forceinline__ double* icp_plane_normals(const IcpGridView& ga, long long n2) { return reinterpret_cast<double*>(ga.ws + icp_plane_normals_off(n2)); }
__device__ __forceinline__ int* icp_plane_counts(const IcpGridView& ga, long long n2) { return reinterpret_cast<int*>(ga.ws + icp_plane_counts_off(n2)); }

struct IcpPlaneArgs : IcpGridArgs {   // ws_off: pair b's part (grid A at its head)
  int parts;                    // sort / normals: workgroups per pair (blockIdx.x = pair * parts + part)
  const long long* ws_off_b;    // [B] byte offset of pair b's grid B (= ws_off[b] + icp_grid_pair_bytes(n2))
  double normal_radius;
  // read only by the traced instantiations (alignnet_debug_icp_plane: one pair): residual per source point of the first evaluation, its sums, the update
  double* tr_resid; double* tr_sums; double* tr_update;
};

__device__ __forceinline__ double icp_dot3_unfused(double a0, double b0, double a1, double b1, double a2, double b2)
{
#pragma clang fp contract(off)
  return (a0 * b0 + a1 * b1) + a2 * b2;
}
__device__ __forceinline__ double icp_affine_unfused(double t0, double t1, double t2, double t3, double x, double y, double z)
{
#pragma clang fp contract(off)
  return ((t0 * x + t1 * y) + t2 * z) + t3;
}

// grid B's records in original-index order inside every bucket: one lane per record finds its bucket again (the build's hash of the build's edge),
// counts the bucket's records of lower index and writes itself there in the second array.  blockIdx.x = pair * parts + part (the pair in x: no
// 65,535 limit on the pairs of a chunk); the parts of a pair stride over its records
// the cloud's grid `g` (n2 records) and where the ordered records go are the caller's
__device__ __forceinline__ void icp_plane_sort_cloud(const IcpGridView& g, float4* srt, long long n2, int part, int parts)
{
  for (long long j = (long long)part * kIcpPlaneLanes + threadIdx.x; j < n2; j += (long long)parts * kIcpPlaneLanes) {
    const float4 q = g.rec[j];
    const int mine = __float_as_int(q.w);
    const unsigned hb = icp_grid_bucket((double)q.x, (double)q.y, (double)q.z, g.edge, g.mask);
    const int lo = g.start[hb], hi = g.start[hb + 1];
    int rank = 0;
    for (int k = lo; k < hi; ++k) rank += __float_as_int(g.rec[k].w) < mine ? 1 : 0;
    if (j >= lo && j < hi) srt[lo + rank] = q;   // (always: the record sits in the bucket its coordinates hash to)
  }
}

__global__ __launch_bounds__(kIcpPlaneLanes) void icp_plane_sort_kernel(const IcpPlaneArgs a)
{
  const int b = blockIdx.x / a.parts, part = blockIdx.x % a.parts;
  const long long row = a.rows ? a.rows[b] : b;
  const long long n2 = a.off[(row + 1) * 2 + 1] - a.off[row * 2 + 1];
  const IcpGridView g = icp_grid_view(a.ws + a.ws_off_b[b], n2);   // grid B
  float4* const srt = icp_plane_sorted(icp_grid_view(a.ws + a.ws_off[b], n2), n2);   // (behind the pair's grid A)
  icp_plane_sort_cloud(g, srt, n2, part, a.parts);
}

// normals and neighbour counts of the cloud `dst` [n2][3] from its grid `g` and the index-ordered records `srt`
__device__ __forceinline__ void icp_plane_normals_cloud(const float* dst, long long n2, const IcpGridView& g, const float4* srt, double* nrm, int* cnt,
                                                        double normal_radius, int part, int parts)
{
  const double r2 = normal_radius * normal_radius;
  for (long long i = (long long)part * kIcpPlaneLanes + threadIdx.x; i < n2; i += (long long)parts * kIcpPlaneLanes) {
    const double qx = (double)dst[i * 3], qy = (double)dst[i * 3 + 1], qz = (double)dst[i * 3 + 2];
    const int gx = icp_grid_cell(qx, g.edge), gy = icp_grid_cell(qy, g.edge), gz = icp_grid_cell(qz, g.edge);
    int K = 0;
    double s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
#pragma unroll 1
    for (int c = 0; c < 27; ++c) {
      const unsigned hb = icp_grid_hash(gx + c % 3 - 1, gy + (c / 3) % 3 - 1, gz + c / 9 - 1) & g.mask;
      bool seen = false;   // an earlier cell in the same bucket: walked already
#pragma unroll 1
      for (int c0 = 0; c0 < c; ++c0) seen = seen || (icp_grid_hash(gx + c0 % 3 - 1, gy + (c0 / 3) % 3 - 1, gz + c0 / 9 - 1) & g.mask) == hb;
      if (seen) continue;
      const int lo = g.start[hb], hi = g.start[hb + 1];
#pragma unroll 1
      for (int j = lo; j < hi; ++j) {
        const float4 q = srt[j];
        const double dx = (double)q.x - qx, dy = (double)q.y - qy, dz = (double)q.z - qz;
        const double d = dx * dx + dy * dy + dz * dz;
        if (d <= r2) {
          ++K;
          s1x += dx; s1y += dy; s1z += dz;
          sxx += dx * dx; sxy += dx * dy; sxz += dx * dz; syy += dy * dy; syz += dy * dz; szz += dz * dz;
        }
      }
    }
    double n[3] = {0.0, 0.0, 1.0};
    if (K >= 3) {
      const double k = (double)K, mx = s1x / k, my = s1y / k, mz = s1z / k;
      icp_smallest_eigenvector(sxx / k - mx * mx, sxy / k - mx * my, sxz / k - mx * mz, syy / k - my * my, syz / k - my * mz, szz / k - mz * mz, n);
      const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
      if (!(nn > 0.0)) { n[0] = 0.0; n[1] = 0.0; n[2] = 1.0; }
      else { n[0] /= nn; n[1] /= nn; n[2] /= nn; }
      if (n[2] < 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
    }
    nrm[i * 3] = n[0]; nrm[i * 3 + 1] = n[1]; nrm[i * 3 + 2] = n[2];
    cnt[i] = K;
  }
}

__global__ __launch_bounds__(kIcpPlaneLanes) void icp_plane_normals_kernel(const IcpPlaneArgs a)
{
  const int b = blockIdx.x / a.parts, part = blockIdx.x % a.parts;
  const long long row = a.rows ? a.rows[b] : b;
  const long long t_lo = a.off[row * 2 + 1], n2 = a.off[(row + 1) * 2 + 1] - t_lo;
  const float* dst = a.pts[1] + t_lo * 3;
  const IcpGridView g = icp_grid_view(a.ws + a.ws_off_b[b], n2), ga = icp_grid_view(a.ws + a.ws_off[b], n2);   // grid B; grid A for the arrays
  icp_plane_normals_cloud(dst, n2, g, icp_plane_sorted(ga, n2), icp_plane_normals(ga, n2), icp_plane_counts(ga, n2), a.normal_radius, part, a.parts);
}

// the update U (rows 0..2 of the 4x4) from the reduced sums; false (U = I): nothing determined
template <bool kFull>
__device__ __forceinline__ bool icp_plane_update(const double* tot, double cx, double cy, double cz, double* U)
{
  constexpr int N = kFull ? 6 : 4, TRI = N * (N + 1) / 2;
#pragma unroll
  for (int q = 0; q < 12; ++q) U[q] = q % 5 == 0 ? 1.0 : 0.0;
  if (!(tot[0] > 0.0)) return false;
  double L[N][N], s[N], y[N];
  {
    int q = 2;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = i; j < N; ++j) L[j][i] = tot[q++];   // the lower triangle holds A
  }
  bool ok = true;
#pragma unroll
  for (int i = 0; i < N; ++i) { ok = ok && L[i][i] > 0.0; s[i] = 1.0 / sqrt(L[i][i]); }
  if (!ok) return false;
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) L[i][j] = L[i][j] * s[i] * s[j];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double d = L[k][k];
#pragma unroll
    for (int j = 0; j < k; ++j) d -= L[k][j] * L[k][j];
    if (!(d > kIcpPlanePivot)) return false;
    d = sqrt(d);
    L[k][k] = d;
#pragma unroll
    for (int i = k + 1; i < N; ++i) {
      double v = L[i][k];
#pragma unroll
      for (int j = 0; j < k; ++j) v -= L[i][j] * L[k][j];
      L[i][k] = v / d;
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double v = -(s[i] * tot[2 + TRI + i]);
#pragma unroll
    for (int j = 0; j < i; ++j) v -= L[i][j] * y[j];
    y[i] = v / L[i][i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double v = y[i];
#pragma unroll
    for (int j = i + 1; j < N; ++j) v -= L[j][i] * y[j];
    y[i] = v / L[i][i];
  }
#pragma unroll
  for (int i = 0; i < N; ++i) y[i] *= s[i];
  double R[9], t[3];
  if constexpr (kFull) {
    const double ca = cos(y[0]), sa = sin(y[0]), cb = cos(y[1]), sb = sin(y[1]), cg = cos(y[2]), sg = sin(y[2]);   // Rz(g) Ry(b) Rx(a)
    R[0] = cg * cb; R[1] = cg * sb * sa - sg * ca; R[2] = cg * sb * ca + sg * sa;
    R[3] = sg * cb; R[4] = sg * sb * sa + cg * ca; R[5] = sg * sb * ca - cg * sa;
    R[6] = -sb;     R[7] = cb * sa;                R[8] = cb * ca;
    t[0] = y[3]; t[1] = y[4]; t[2] = y[5];
  } else {
    const double cg = cos(y[0]), sg = sin(y[0]);
    R[0] = cg; R[1] = -sg; R[2] = 0.0; R[3] = sg; R[4] = cg; R[5] = 0.0; R[6] = 0.0; R[7] = 0.0; R[8] = 1.0;
    t[0] = y[1]; t[1] = y[2]; t[2] = y[3];
  }
  const double c[3] = {cx, cy, cz};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    U[r * 4] = R[r * 3]; U[r * 4 + 1] = R[r * 3 + 1]; U[r * 4 + 2] = R[r * 3 + 2];
    U[r * 4 + 3] = (c[r] + t[r]) - (R[r * 3] * c[0] + R[r * 3 + 1] * c[1] + R[r * 3 + 2] * c[2]);   // Tr(c) [R | t] Tr(-c)
  }
  return true;
}

// ---- generalized (plane-to-plane) ICP (alignnet_icp_generalized_register*): normals of BOTH clouds once per call, every correspondence weighted by
// the inverse of the sum of the two surface covariances ---------------------------------------------------------------------------------------------
// Semantics: tests/icp_generalized_ref.py (Segal, Haehnel, Thrun 2009; the covariances of Open3D's registration_generalized_icp, epsilon 1e-3).  A
// point with unit normal n has the covariance C = I - (1 - eps) n n^T, never stored.  Per pair, once per call: what point-to-plane prepares for the
// target (grid A, grid B, ordered records, normals, counts: the same kernels, the same layout at the head of the pair's part) and behind it a third
// grid over the SOURCE with cells of normal_radius, its ordered records, normals and counts (icp_generalized_*_source_kernel: the bodies of the
// target's kernels on the other cloud; the normals are taken in the source's own frame) and one int per source point for the loop.
// Loop (icp_surface_kernel<true, .>, one workgroup of 1024 lanes per pair, bucket starts of grid A in LDS, icp_grid_nearest): evaluate, stop test, estimate,
// T <- U T as point-to-plane.  Estimate over the inliers (p, q, n_q, n_p), R = the rotation of the current T: m = R n_p,
// A = 2 I - (1 - eps)(n_q n_q^T + m m^T) = C_q + R C_p R^T, M = A^-1 by cofactors, d = p - q, a = p - c, J = [e_x x a, e_y x a, e_z x a, I] (full) or
// [e_z x a, I] (z-constrained); the sums are count, sum |d|^2, the upper triangle of sum J^T M J row by row and sum J^T M d: point-to-plane's 16 / 29
// slots, reduced by block_reduce and solved by icp_plane_update as they are.  Everything per correspondence is evaluated without contraction in the
// order the restatement states (icp_generalized_terms), so every term is the restatement's to the last bit; the zeros and ones of J are left out
// (x * 0, x + 0 and x * 1 are exact).
// Registers: the full-rotation point-to-plane kernel spills with its 29 fp64 accumulators in the 128 registers a 1024-lane workgroup leaves a lane,
// and this estimate holds M, W = M J and w = M d beside them.  The full-rotation instantiation therefore takes the matrix sums in TWO PASSES over the
// inliers of a lane (the first of DESIGN.md 4.7d's leads): pass 0 searches, leaves each source point's correspondence (or -1) in the pair's workspace
// and accumulates slots 0..14; pass 1 reads it back, recomputes p, M and W from the same inputs and accumulates slots 15..28.  Each pass ends in its
// own block_reduce (15 and 14 wide), so no accumulator of one pass is live in the other.  The z-constrained instantiation (16 slots) takes one pass.
constexpr double kIcpGenKappa = 1.0 - 1e-3;   // 1 - eps
constexpr int kIcpGenSplit = 15;              // full rotation: slots [0, 15) in pass 0, [15, 29) in pass 1

// a pair's workspace: the point-to-plane layout of the target | source grid | its records, index-ordered [n1] float4 | source normals [n1][3] doubles |
// source neighbour counts [n1] ints | correspondences [n1] ints
__host__ __device__ inline size_t icp_gen_source_off(long long n2) { return icp_plane_pair_bytes(n2); }
__host__ __device__ inline size_t icp_gen_sorted_off(long long n1) { return icp_grid_pair_bytes(n1); }   // (from the source part's head)
__host__ __device__ inline size_t icp_gen_normals_off(long long n1) { return icp_gen_sorted_off(n1) + icp_r256((size_t)n1 * 16); }
__host__ __device__ inline size_t icp_gen_counts_off(long long n1) { return icp_gen_normals_off(n1) + icp_r256((size_t)n1 * 24); }
__host__ __device__ inline size_t icp_gen_corr_off(long long n1) { return icp_gen_counts_off(n1) + icp_r256((size_t)n1 * 4); }
__host__ __device__ inline size_t icp_gen_pair_bytes(long long n1, long long n2) { return icp_gen_source_off(n2) + icp_gen_corr_off(n1) + icp_r256((size_t)n1 * 4); }

// the three source kernels: blockIdx.x = pair for the build, pair * parts + part for the other two (IcpPlaneArgs as the target's kernels take it)
__global__ __launch_bounds__(kIcpThreads) void icp_generalized_build_source_kernel(const IcpPlaneArgs a)
{
  const int b = blockIdx.x;
  const IcpPair pr = icp_pair(a, b);
  icp_grid_build_cloud(a.pts[0] + pr.s_lo * 3, pr.n1, a.ws + a.ws_off[b] + icp_gen_source_off(pr.n2), a.normal_radius);
}

__global__ __launch_bounds__(kIcpPlaneLanes) void icp_generalized_sort_source_kernel(const IcpPlaneArgs a)
{
  const int b = blockIdx.x / a.parts, part = blockIdx.x % a.parts;
  const long long row = a.rows ? a.rows[b] : b;
  const long long n1 = a.off[(row + 1) * 2] - a.off[row * 2], n2 = a.off[(row + 1) * 2 + 1] - a.off[row * 2 + 1];
  char* const ws = a.ws + a.ws_off[b] + icp_gen_source_off(n2);
  icp_plane_sort_cloud(icp_grid_view(ws, n1), reinterpret_cast<float4*>(ws + icp_gen_sorted_off(n1)), n1, part, a.parts);
}

__global__ __launch_bounds__(kIcpPlaneLanes) void icp_generalized_normals_source_kernel(const IcpPlaneArgs a)
{
  const int b = blockIdx.x / a.parts, part = blockIdx.x % a.parts;
  const long long row = a.rows ? a.rows[b] : b;
  const long long s_lo = a.off[row * 2], n1 = a.off[(row + 1) * 2] - s_lo;
  const long long n2 = a.off[(row + 1) * 2 + 1] - a.off[row * 2 + 1];
  char* const ws = a.ws + a.ws_off[b] + icp_gen_source_off(n2);
  icp_plane_normals_cloud(a.pts[0] + s_lo * 3, n1, icp_grid_view(ws, n1), reinterpret_cast<const float4*>(ws + icp_gen_sorted_off(n1)),
                          reinterpret_cast<double*>(ws + icp_gen_normals_off(n1)), reinterpret_cast<int*>(ws + icp_gen_counts_off(n1)), a.normal_radius,
                          part, a.parts);
}

// column k of J's rotation block (e_k x a) times the vector x, its zero left out: (0, -a_z, a_y), (a_z, 0, -a_x), (-a_y, a_x, 0)
__device__ __forceinline__ double icp_gen_rotdot(int k, double ax, double ay, double az, double x0, double x1, double x2)
{
#pragma clang fp contract(off)
  return k == 0 ? (-az) * x1 + ay * x2 : k == 1 ? az * x0 + (-ax) * x2 : (-ay) * x0 + ax * x1;
}

// the terms of one correspondence in the slots [kLo, kHi) added onto v[0 .. kHi - kLo): p, q the points, nq / np the target's and the source's normal,
// T the current transform (its rotation turns np), c the pivot, best the squared distance.  No contraction, the restatement's order
template <bool kFull, int kLo, int kHi>
__device__ __forceinline__ void icp_generalized_terms(double px, double py, double pz, double qx, double qy, double qz, const double* nq, const double* np,
                                                      const double* T, double cx, double cy, double cz, double best, double (&v)[kHi - kLo])
{
#pragma clang fp contract(off)
  constexpr int N = kFull ? 6 : 4, R = kFull ? 3 : 1, kRot0 = kFull ? 0 : 2;   // columns; rotation columns; the axis of the first of them
  const double m0 = (T[0] * np[0] + T[1] * np[1]) + T[2] * np[2];
  const double m1 = (T[4] * np[0] + T[5] * np[1]) + T[6] * np[2];
  const double m2 = (T[8] * np[0] + T[9] * np[1]) + T[10] * np[2];
  const double a00 = 2.0 - kIcpGenKappa * (nq[0] * nq[0] + m0 * m0), a01 = -(kIcpGenKappa * (nq[0] * nq[1] + m0 * m1));
  const double a02 = -(kIcpGenKappa * (nq[0] * nq[2] + m0 * m2)), a11 = 2.0 - kIcpGenKappa * (nq[1] * nq[1] + m1 * m1);
  const double a12 = -(kIcpGenKappa * (nq[1] * nq[2] + m1 * m2)), a22 = 2.0 - kIcpGenKappa * (nq[2] * nq[2] + m2 * m2);
  const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
  const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
  const double det = (a00 * c00 + a01 * c01) + a02 * c02;
  double M[3][3];
  M[0][0] = c00 / det; M[0][1] = M[1][0] = c01 / det; M[0][2] = M[2][0] = c02 / det;
  M[1][1] = c11 / det; M[1][2] = M[2][1] = c12 / det; M[2][2] = c22 / det;
  const double dx = px - qx, dy = py - qy, dz = pz - qz, ax = px - cx, ay = py - cy, az = pz - cz;
  double W[3][N], w[3];   // M J, M d
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < R; ++k) W[r][k] = icp_gen_rotdot(kRot0 + k, ax, ay, az, M[r][0], M[r][1], M[r][2]);
#pragma unroll
    for (int j = 0; j < 3; ++j) W[r][R + j] = M[r][j];
    w[r] = (M[r][0] * dx + M[r][1] * dy) + M[r][2] * dz;
  }
  double t[kFull ? kIcpPlaneSumsFull : kIcpPlaneSums];
  t[0] = 1.0; t[1] = best;
  int q = 2;
#pragma unroll
  for (int k = 0; k < N; ++k)
#pragma unroll
    for (int l = k; l < N; ++l) t[q++] = k < R ? icp_gen_rotdot(kRot0 + k, ax, ay, az, W[0][l], W[1][l], W[2][l]) : W[k - R][l];
#pragma unroll
  for (int k = 0; k < N; ++k) t[q++] = k < R ? icp_gen_rotdot(kRot0 + k, ax, ay, az, w[0], w[1], w[2]) : w[k - R];
#pragma unroll
  for (int s = kLo; s < kHi; ++s) v[s - kLo] += t[s];
}

// The loop of both normal-equation estimates: kGen = false point-to-plane (its terms stand in the loop), kGen = true generalized (icp_generalized_terms, and with
// kFull its second pass); everything around the terms of a correspondence is one source.
// kTrace (alignnet_debug_icp_plane / _generalized, one pair): the same evaluation with one record per source point behind it, then the sums and the
// update of the estimate that follows, and no further iteration
template <bool kGen, bool kFull, bool kTrace = false>
__global__ __launch_bounds__(kIcpThreads) void icp_surface_kernel(const IcpPlaneArgs a)
{
  constexpr int kSums = kFull ? kIcpPlaneSumsFull : kIcpPlaneSums, kFirst = kGen && kFull ? kIcpGenSplit : kSums;   // kFirst: the slots of pass 0
  extern __shared__ __attribute__((aligned(16))) int gstart[];   // [H + 1] bucket starts of grid A
  __shared__ double T[12];
  __shared__ double red[(kIcpThreads / 64) * kFirst], tot[kSums];
  const int b = blockIdx.x, tid = threadIdx.x;
  const IcpPair pr = icp_pair(a, b);
  const long long n1 = pr.n1, n2 = pr.n2;
  const float* src = a.pts[0] + pr.s_lo * 3;
  const float* dst = a.pts[1] + pr.t_lo * 3;
  if (tid < 12) T[tid] = a.init[(size_t)b * 16 + tid];
  IcpGridView g = icp_grid_view(a.ws + a.ws_off[b], n2);
  const double* const nrm = icp_plane_normals(g, n2);
  [[maybe_unused]] const double* snrm = nullptr;   // kGen: the source's normals and the correspondences of pass 0 (point-to-plane has no source part)
  [[maybe_unused]] int* corr = nullptr;
  if constexpr (kGen) {
    const char* const sws = g.ws + icp_gen_source_off(n2);
    snrm = reinterpret_cast<const double*>(sws + icp_gen_normals_off(n1));
    corr = reinterpret_cast<int*>(g.ws + icp_gen_source_off(n2) + icp_gen_corr_off(n1));
  }
  for (int j = tid; j <= g.buckets; j += kIcpThreads) gstart[j] = g.start[j];
  g.start = gstart;   // the search reads the LDS copy
  __syncthreads();
  const double r2 = a.radius * a.radius;
  const double cx = n2 > 0 ? (double)dst[0] : 0.0, cy = n2 > 0 ? (double)dst[1] : 0.0, cz = n2 > 0 ? (double)dst[2] : 0.0;   // the pivot of icp_kernel
  double fit_prev = 0.0, rmse_prev = 0.0, fit = 0.0, rmse = 0.0;
  int k = 0;
  if (n1 > 0 && n2 > 0)
    for (k = 0;; ++k) {
      {
        double v[kFirst];
#pragma unroll
        for (int q = 0; q < kFirst; ++q) v[q] = 0.0;
        for (long long i = tid; i < n1; i += kIcpThreads) {
          const double sx = src[i * 3], sy = src[i * 3 + 1], sz = src[i * 3 + 2];
          const double px = icp_affine_unfused(T[0], T[1], T[2], T[3], sx, sy, sz);
          const double py = icp_affine_unfused(T[4], T[5], T[6], T[7], sx, sy, sz);
          const double pz = icp_affine_unfused(T[8], T[9], T[10], T[11], sx, sy, sz);
          double best = 1e300; int bj = 0x7fffffff;
          float4 brec = {0.f, 0.f, 0.f, 0.f};
          int cand = 0;   // (counted by icp_kernel's traced instantiation alone)
          icp_grid_nearest<false>(px, py, pz, g, best, bj, brec, cand);
          const bool inlier = best <= r2;
          [[maybe_unused]] double res = 0.0;
          if constexpr (kGen && kFull) corr[i] = inlier ? bj : -1;
          if (inlier) {
            if constexpr (kGen)
              icp_generalized_terms<kFull, 0, kFirst>(px, py, pz, (double)brec.x, (double)brec.y, (double)brec.z, nrm + (size_t)bj * 3, snrm + (size_t)i * 3, T,
                                                      cx, cy, cz, best, v);
            else
            {   // point-to-plane's terms, written out here: as a function like icp_generalized_terms they compile to another order
              const double nx = nrm[(size_t)bj * 3], ny = nrm[(size_t)bj * 3 + 1], nz = nrm[(size_t)bj * 3 + 2];
              res = icp_dot3_unfused(px - (double)brec.x, nx, py - (double)brec.y, ny, pz - (double)brec.z, nz);
              const double ax = px - cx, ay = py - cy, az = pz - cz;
              v[0] += 1.0; v[1] += best;
              if constexpr (kFull) {
                const double J[6] = {ay * nz - az * ny, az * nx - ax * nz, ax * ny - ay * nx, nx, ny, nz};
                int q = 2;
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                  for (int j = i; j < 6; ++j) v[q++] += J[i] * J[j];
#pragma unroll
                for (int i = 0; i < 6; ++i) v[23 + i] += J[i] * res;
              } else {
                const double J[4] = {ax * ny - ay * nx, nx, ny, nz};
                int q = 2;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                  for (int j = i; j < 4; ++j) v[q++] += J[i] * J[j];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[12 + i] += J[i] * res;
              }
            }
          }
          if constexpr (kTrace) {
            if (k == 0) {
              const bool found = bj != 0x7fffffff;
              a.tr_index[i] = found ? bj : -1; a.tr_dist[i] = found ? best : __builtin_huge_val(); a.tr_inlier[i] = inlier;
              if constexpr (!kGen) a.tr_resid[i] = res;
            }
          }
        }
        block_reduce(v, red, tot);
      }
      if constexpr (kGen && kFull) {   // pass 1: the lane's own correspondences again, the other slots
        double v[kSums - kFirst];
#pragma unroll
        for (int q = 0; q < kSums - kFirst; ++q) v[q] = 0.0;
        for (long long i = tid; i < n1; i += kIcpThreads) {
          const int bj = corr[i];
          if (bj < 0) continue;
          const double sx = src[i * 3], sy = src[i * 3 + 1], sz = src[i * 3 + 2];
          const double px = icp_affine_unfused(T[0], T[1], T[2], T[3], sx, sy, sz);
          const double py = icp_affine_unfused(T[4], T[5], T[6], T[7], sx, sy, sz);
          const double pz = icp_affine_unfused(T[8], T[9], T[10], T[11], sx, sy, sz);
          icp_generalized_terms<kFull, kFirst, kSums>(px, py, pz, (double)dst[(size_t)bj * 3], (double)dst[(size_t)bj * 3 + 1], (double)dst[(size_t)bj * 3 + 2],
                                                      nrm + (size_t)bj * 3, snrm + (size_t)i * 3, T, cx, cy, cz, 0.0, v);
        }
        block_reduce(v, red, tot + kFirst);
      }
      const double cnt = tot[0];
      fit = cnt / (double)n1;
      rmse = cnt > 0.0 ? sqrt(tot[1] / cnt) : 0.0;
      if constexpr (kTrace) {
        if (tid == 0) {
          double U[12];
          icp_plane_update<kFull>(tot, cx, cy, cz, U);
          for (int q = 0; q < kIcpPlaneSumsFull; ++q) a.tr_sums[q] = q < kSums ? tot[q] : 0.0;
          for (int q = 0; q < 12; ++q) a.tr_update[q] = U[q];
        }
        break;
      }
      if (k > 0 && fabs(fit - fit_prev) < 1e-6 && fabs(rmse - rmse_prev) < 1e-6) break;
      if (k == a.its) break;
      fit_prev = fit; rmse_prev = rmse;
      if (tid == 0) {
        double U[12], n[12];
        if (icp_plane_update<kFull>(tot, cx, cy, cz, U)) {   // T <- U T
#pragma unroll
          for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int col = 0; col < 4; ++col) n[r * 4 + col] = U[r * 4] * T[col] + U[r * 4 + 1] * T[4 + col] + U[r * 4 + 2] * T[8 + col];
            n[r * 4 + 3] += U[r * 4 + 3];
          }
          for (int q = 0; q < 12; ++q) T[q] = n[q];
        }
      }
      __syncthreads();
    }
  __syncthreads();
  if (tid < 12) a.out[(size_t)b * 16 + tid] = T[tid];
  if (tid >= 12 && tid < 16) a.out[(size_t)b * 16 + tid] = tid == 15 ? 1.0 : 0.0;
  if (tid == 0) {
    if (a.fitness) a.fitness[b] = fit;
    if (a.rmse) a.rmse[b] = rmse;
    if (a.iters) a.iters[b] = k;
  }
}

using Loop = void (*)(const IcpPlaneArgs);
constexpr Loop kIcpSurface[2][2][2] = {   // [gen][trace][full]
    {{icp_surface_kernel<false, false>, icp_surface_kernel<false, true>}, {icp_surface_kernel<false, false, true>, icp_surface_kernel<false, true, true>}},
    {{icp_surface_kernel<true, false>, icp_surface_kernel<true, true>}, {icp_surface_kernel<true, false, true>, icp_surface_kernel<true, true, true>}}};

// alignnet_debug_icp_plane / _generalized: host arrays of the one pair (resid: point-to-plane; src_normals / src_neighbours: generalized; else null)
struct IcpPlaneTrace {
  long long n1, n2; double* normals; int* neighbours; int* index; double* dist; int* inlier; double* resid; double* sums; double* update;
  double* src_normals = nullptr; int* src_neighbours = nullptr;
};

// shared driver of the point-to-plane and (gen) the generalized entry points: clouds already on the device
int run_icp_plane(alignnet_handle* h, const IcpClouds& c, int B, const double* init, double radius, double normal_radius, int its, bool full, bool gen,
                  double* out, double* fitness, double* rmse, int* iters, const IcpPlaneTrace* trace = nullptr, const alignnet::IcpDeviceIo* dev = nullptr)
{
  // dev: as in run_icp
  const std::vector<long long>& n2 = c.n2;
  const std::vector<long long>& n1 = c.n1;   // (read by the generalized estimate alone)
  const std::string what(gen ? "icp_generalized" : "icp_plane");
  if (!init || !out) return fail(h, what + ": null init / out");
  if (!(radius > 0.0) || !(normal_radius > 0.0) || its < 0) return fail(h, what + ": radius and normal_radius must be > 0 and its >= 0");
  if (gen && (int)n1.size() != B) return fail(h, what + ": the source sizes are not known");
  // consecutive pairs form chunks of at most kIcpGridWsBudget of workspace (two grids, the ordered records, normals and counts per pair, and with gen the
  // source's part behind them; one pair may exceed it alone); every chunk reuses the handle's workspace -- the grid search's -- in stream order
  std::vector<long long> ws_off_own;
  std::vector<long long>& ws_off = dev ? *dev->h_ws_off : ws_off_own;
  ws_off.assign(2 * (size_t)B, 0);
  std::vector<int> first;   // the chunks' first pairs
  const size_t own_budget = gen ? h->icp_generalized_ws_budget : h->icp_plane_ws_budget, budget = own_budget ? own_budget : kIcpGridWsBudget;
  constexpr int kChunkPairs = 1 << 20;   // pairs x parts (<= 1024) of a chunk stay a valid gridDim.x
  size_t need = 0, cur = 0;
  for (int b = 0; b < B; ++b) {
    if (n2[b] > 0x7fffffff) return fail(h, what + ": more than 2^31 - 1 target points in a pair");
    if (gen && n1[b] > 0x7fffffff) return fail(h, what + ": more than 2^31 - 1 source points in a pair");
    const size_t bytes = gen ? icp_gen_pair_bytes(n1[b], n2[b]) : icp_plane_pair_bytes(n2[b]);
    if (b == 0 || cur + bytes > budget || b - first.back() >= kChunkPairs) { first.push_back(b); cur = 0; }
    ws_off[b] = (long long)cur; ws_off[(size_t)B + b] = (long long)(cur + icp_grid_pair_bytes(n2[b]));
    cur += bytes;
    need = std::max(need, cur);
  }
  first.push_back(B);
  (gen ? h->icp_generalized_chunks : h->icp_plane_chunks) = (int)first.size() - 1;
  if (reserve_grid_ws(h, need)) return 1;
  IcpPlaneArgs a;
  IcpResults res;
  DevBuf<long long> wsoff;
  DevBuf<double> trd; DevBuf<int> tri;   // the read-back's records
  if (dev) { a.init = init; a.out = out; a.fitness = fitness; a.rmse = rmse; a.iters = iters; }
  else if (res.up(h, B, init, &a)) return 1;
  if (!dev) HIP_TRY(h, wsoff.alloc((size_t)B * 2));
  long long* const d_ws_off = dev ? dev->ws_off : wsoff.p;
  HIP_TRY(h, hipMemcpyAsync(d_ws_off, ws_off.data(), (size_t)B * 2 * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  a.pts[0] = c.pts[0]; a.pts[1] = c.pts[1]; a.off = c.off; a.rows = c.rows; a.radius = radius; a.its = its; a.lds_points = 0;
  a.tr_index = a.tr_inlier = a.tr_paths = nullptr; a.tr_dist = a.tr_resid = a.tr_sums = a.tr_update = nullptr;
  a.ws = static_cast<char*>(h->icp_grid_ws); a.ws_off = d_ws_off; a.ws_off_b = d_ws_off + B; a.normal_radius = normal_radius; a.parts = 1;
  const size_t tn = trace ? (size_t)std::max<long long>(trace->n1, 1) : 0;
  if (trace) {   // doubles: dist [n1] | residual [n1] | sums [29] | update [12]; ints: index [n1] | inlier [n1]
    HIP_TRY(h, trd.alloc(2 * tn + kIcpPlaneSumsFull + 12));
    HIP_TRY(h, tri.alloc(2 * tn));
    HIP_TRY(h, hipMemsetAsync(trd.p, 0, (2 * tn + kIcpPlaneSumsFull + 12) * sizeof(double), h->stream));
    HIP_TRY(h, hipMemsetAsync(tri.p, 0xff, tn * sizeof(int), h->stream));   // (index -1 where the kernel wrote nothing: an empty target)
    HIP_TRY(h, hipMemsetAsync(tri.p + tn, 0, tn * sizeof(int), h->stream));
    a.tr_dist = trd.p; a.tr_resid = trd.p + tn; a.tr_sums = trd.p + 2 * tn; a.tr_update = a.tr_sums + kIcpPlaneSumsFull;
    a.tr_index = tri.p; a.tr_inlier = tri.p + tn;
  }
  static alignnet::PerDeviceOnce attr[8];
  const int slot = (full ? 1 : 0) + (trace ? 2 : 0) + (gen ? 4 : 0);
  const Loop loop = kIcpSurface[gen][trace != nullptr][full];
  if (attr[slot].need(h->cfg.device)) {
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(loop), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096));
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(icp_grid_build_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096));
    if (gen)
      HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(icp_generalized_build_source_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     160 * 1024 - 4096));
    attr[slot].mark(h->cfg.device);
  }
  for (size_t c = 0; c + 1 < first.size(); ++c) {
    const int lo = first[c], hi = first[c + 1];
    const long long big = *std::max_element(n2.begin() + lo, n2.begin() + hi);
    IcpPlaneArgs r = icp_args_from<IcpPlaneArgs>(a, lo);
    r.ws_off += lo; r.ws_off_b += lo;
    const size_t lds = ((size_t)icp_grid_buckets(big) + 1) * 4;
    IcpGridArgs ga = r, gb = r;
    gb.radius = normal_radius; gb.ws_off = r.ws_off_b;
    const long long big1 = gen ? *std::max_element(n1.begin() + lo, n1.begin() + hi) : 0;   // the chunk's largest source
    {
      alignnet::ProfScope prof_scope(h, alignnet::PK_ICP_GRID_BUILD);
      hipLaunchKernelGGL(icp_grid_build_kernel, dim3(hi - lo), dim3(kIcpThreads), lds, h->stream, ga);
      hipLaunchKernelGGL(icp_grid_build_kernel, dim3(hi - lo), dim3(kIcpThreads), lds, h->stream, gb);
      if (gen)
        hipLaunchKernelGGL(icp_generalized_build_source_kernel, dim3(hi - lo), dim3(kIcpThreads), ((size_t)icp_grid_buckets(big1) + 1) * 4, h->stream, r);
    }
    if (big > 0) {
      // the parts per pair are sized by the chunk's largest target: a small pair beside a large one launches workgroups that find nothing to do
      alignnet::ProfScope prof_scope(h, gen ? alignnet::PK_ICP_GENERALIZED_NORMALS : alignnet::PK_ICP_PLANE_NORMALS);
      r.parts = (int)std::min<long long>((big + kIcpPlaneLanes - 1) / kIcpPlaneLanes, kIcpPlaneMaxBlocks);
      const dim3 blocks((unsigned)r.parts * (unsigned)(hi - lo));
      hipLaunchKernelGGL(icp_plane_sort_kernel, blocks, dim3(kIcpPlaneLanes), 0, h->stream, r);
      hipLaunchKernelGGL(icp_plane_normals_kernel, blocks, dim3(kIcpPlaneLanes), 0, h->stream, r);
    }
    if (big1 > 0) {   // the source's, its parts sized by the chunk's largest source
      alignnet::ProfScope prof_scope(h, alignnet::PK_ICP_GENERALIZED_NORMALS);
      r.parts = (int)std::min<long long>((big1 + kIcpPlaneLanes - 1) / kIcpPlaneLanes, kIcpPlaneMaxBlocks);
      const dim3 blocks((unsigned)r.parts * (unsigned)(hi - lo));
      hipLaunchKernelGGL(icp_generalized_sort_source_kernel, blocks, dim3(kIcpPlaneLanes), 0, h->stream, r);
      hipLaunchKernelGGL(icp_generalized_normals_source_kernel, blocks, dim3(kIcpPlaneLanes), 0, h->stream, r);
    }
    alignnet::ProfScope prof_scope(h, gen ? alignnet::PK_ICP_GENERALIZED : alignnet::PK_ICP_PLANE);
    hipLaunchKernelGGL(loop, dim3(hi - lo), dim3(kIcpThreads), lds, h->stream, r);
    HIP_TRY(h, hipGetLastError());
  }
  if (trace) {
    const size_t m = (size_t)trace->n1, t2 = (size_t)trace->n2;
    const char* const base = static_cast<const char*>(h->icp_grid_ws);
    if (t2) {
      HIP_TRY(h, hipMemcpyAsync(trace->normals, base + icp_plane_normals_off(trace->n2), t2 * 24, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipMemcpyAsync(trace->neighbours, base + icp_plane_counts_off(trace->n2), t2 * 4, hipMemcpyDeviceToHost, h->stream));
    }
    if (gen && m) {   // (one pair: its source part sits behind the target's)
      const char* const sws = base + icp_gen_source_off(trace->n2);
      HIP_TRY(h, hipMemcpyAsync(trace->src_normals, sws + icp_gen_normals_off(trace->n1), m * 24, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipMemcpyAsync(trace->src_neighbours, sws + icp_gen_counts_off(trace->n1), m * 4, hipMemcpyDeviceToHost, h->stream));
    }
    if (m) {
      HIP_TRY(h, hipMemcpyAsync(trace->dist, trd.p, m * 8, hipMemcpyDeviceToHost, h->stream));
      if (trace->resid) HIP_TRY(h, hipMemcpyAsync(trace->resid, trd.p + tn, m * 8, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipMemcpyAsync(trace->index, tri.p, m * 4, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipMemcpyAsync(trace->inlier, tri.p + tn, m * 4, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(h, hipMemcpyAsync(trace->sums, trd.p + 2 * tn, kIcpPlaneSumsFull * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(trace->update, trd.p + 2 * tn + kIcpPlaneSumsFull, 12 * 8, hipMemcpyDeviceToHost, h->stream));
  }
  if (dev) return 0;
  return res.down(h, B, out, fitness, rmse, iters);
}

int icp_plane_host(alignnet_handle* h, const char* fn, const float* points1, const float* points2, const int64_t* offsets, int32_t B, const double* init,
                   double radius, double normal_radius, int32_t its, bool full, bool gen, double* out, double* fitness, double* rmse, int32_t* iterations,
                   const IcpPlaneTrace* trace = nullptr)
{
  IcpClouds c;
  if (stage_host(h, fn, points1, points2, offsets, B, &c)) return 1;
  return run_icp_plane(h, c, B, init, radius, normal_radius, its, full, gen, out, fitness, rmse, iterations, trace);
}

// what every entry point with flags checks first: the handle, then the flags of alignnet_icp_register* (bit 0 = full rotation; no other bit is defined)
int icp_flags(alignnet_handle* h, const std::string& fn, int32_t flags, bool* full)
{
  if (!h) return 1;
  if (flags & ~1) return fail(h, fn + ": unknown flags " + std::to_string(flags) + " (bit 0 = full rotation is the only one)");
  *full = (flags & 1) != 0;
  return 0;
}

// the read-backs of one pair (alignnet_debug_icp_*): handle, flags, the sizes' range; off: the pair's offsets table
int debug_arguments(alignnet_handle* h, const std::string& fn, int32_t flags, int64_t n1, int64_t n2, bool* full, int64_t* off /*[4]*/)
{
  if (icp_flags(h, fn, flags, full)) return 1;
  if (n1 < 0 || n2 < 0 || n1 > 0x7fffffff || n2 > 0x7fffffff) return fail(h, fn + ": n1 / n2 out of range");
  off[0] = off[1] = 0; off[2] = n1; off[3] = n2;
  return 0;
}

// the traced kernel's update (rows 0..2) as the 4x4 the read-backs return; ran = false (an empty cloud: no evaluation, no update): the identity
void debug_update(const double* up /*[12]*/, bool ran, double* update /*[16]*/)
{
  for (int q = 0; q < 16; ++q) update[q] = q < 12 && ran ? up[q] : (q % 5 == 0 ? 1.0 : 0.0);
}

}  // namespace

int alignnet_icp_run_device(alignnet_handle* h, const float* const pts[2], const long long* off, const int* rows, const long long* n1, const long long* n2,
                            long long stage_n2, int B, const alignnet::IcpDeviceIo& io, double radius, double normal_radius, int its, bool full, int estimate)
{
  if (!h) return 1;
  if (!pts[0] || !pts[1] || !off || (estimate == 4 && !n1) || !n2 || B < 1 || !io.ws_off || !io.h_ws_off) return fail(h, "icp: null device argument or B < 1");
  IcpClouds c;   // (nothing of it is uploaded here: its buffers stay empty)
  c.pts[0] = pts[0]; c.pts[1] = pts[1]; c.off = off; c.rows = rows;
  c.n2.assign(n2, n2 + B);
  if (n1) c.n1.assign(n1, n1 + B);
  if (estimate >= 2)
    return run_icp_plane(h, c, B, io.init, radius, normal_radius, its, full, estimate == 4, io.out, io.fitness, io.rmse, io.iters, nullptr, &io);
  return run_icp(h, c, stage_n2 > 0 ? stage_n2 : kIcpLdsBudget, B, io.init, radius, its, full, io.out, io.fitness, io.rmse, io.iters, nullptr, &io);
}

extern "C" int alignnet_icp_refine(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets, int32_t B,
                                   const double* init, double radius, int32_t its, double* out, double* fitness, double* rmse,
                                   int32_t* iterations)
{
  return icp_host(h, "alignnet_icp_refine", points1, points2, offsets, B, init, radius, its, false, out, fitness, rmse, iterations);
}

extern "C" int alignnet_icp_refine_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, const double* init, double radius,
                                           int32_t its, double* out, double* fitness, double* rmse, int32_t* iterations)
{
  return icp_rows(h, "alignnet_icp_refine_dataset", rows, B, init, radius, its, false, out, fitness, rmse, iterations);
}

extern "C" int alignnet_icp_register(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets, int32_t B,
                                     const double* init, double radius, int32_t its, int32_t flags, double* out, double* fitness, double* rmse,
                                     int32_t* iterations)
{
  bool full = false;
  if (icp_flags(h, "alignnet_icp_register", flags, &full)) return 1;
  return icp_host(h, "alignnet_icp_register", points1, points2, offsets, B, init, radius, its, full, out, fitness, rmse, iterations);
}

extern "C" int alignnet_icp_register_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, const double* init, double radius,
                                             int32_t its, int32_t flags, double* out, double* fitness, double* rmse, int32_t* iterations)
{
  bool full = false;
  if (icp_flags(h, "alignnet_icp_register_dataset", flags, &full)) return 1;
  return icp_rows(h, "alignnet_icp_register_dataset", rows, B, init, radius, its, full, out, fitness, rmse, iterations);
}

extern "C" int alignnet_evaluate_registration(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets, int32_t B,
                                              const double* transforms, double threshold, const double* centers, double* fitness, double* rmse,
                                              double* information, int32_t* correspondences)
{
  if (!h) return 1;
  const std::string name("alignnet_evaluate_registration");
  if (eval_arguments(h, name, B, transforms, threshold, fitness, rmse)) return 1;
  IcpClouds c;
  if (stage_host(h, name.c_str(), points1, points2, offsets, B, &c)) return 1;
  std::vector<long long> corr_off(B);
  for (int b = 0; b < B; ++b) corr_off[b] = offsets[(size_t)b * 2] - offsets[0];   // the offsets table's source ranges
  return run_eval(h, c, *std::max_element(c.n2.begin(), c.n2.end()), B, transforms, threshold, centers, fitness, rmse, information, correspondences,
                  corr_off, offsets[(size_t)B * 2] - offsets[0]);
}

extern "C" int alignnet_evaluate_registration_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, const double* transforms, double threshold,
                                                      const double* centers, double* fitness, double* rmse, double* information,
                                                      int32_t* correspondences)
{
  if (!h) return 1;
  const std::string name("alignnet_evaluate_registration_dataset");
  if (eval_arguments(h, name, B, transforms, threshold, fitness, rmse)) return 1;
  IcpClouds c;
  if (stage_rows(h, name, rows, B, &c)) return 1;
  alignnet::DatasetTables t;
  alignnet_dataset_tables(h, &t);
  std::vector<long long> corr_off(B);
  long long total = 0;   // the rows' source ranges back to back
  for (int b = 0; b < B; ++b) { corr_off[b] = total; total += t.h_off[((size_t)rows[b] + 1) * 2] - t.h_off[(size_t)rows[b] * 2]; }
  return run_eval(h, c, kIcpLdsBudget, B, transforms, threshold, centers, fitness, rmse, information, correspondences, corr_off, total);
}

extern "C" int alignnet_debug_icp_scan(alignnet_handle* h, const float* points1, int64_t n1, const float* points2, int64_t n2, const double* T,
                                       double radius, int32_t flags, int32_t lds_points, int32_t* index, double* dist2, int32_t* inlier,
                                       int32_t* paths, int32_t* lds_points_used, double* fitness, double* rmse)
{
  const std::string name("alignnet_debug_icp_scan");
  bool full = false;
  int64_t off[4];
  if (debug_arguments(h, name, flags, n1, n2, &full, off)) return 1;
  if (lds_points < 0 || lds_points > kIcpLdsBudget) return fail(h, name + ": lds_points must be in [0, " + std::to_string(kIcpLdsBudget) + "] (0 = as shipped)");
  if (!index || !dist2 || !inlier || !paths || !lds_points_used) return fail(h, name + ": null output");
  const IcpTraceOut tr = {n1, lds_points, index, dist2, inlier, paths, lds_points_used, false, nullptr};
  double out[16];
  return icp_host(h, name.c_str(), points1, points2, off, 1, T, radius, 0, full, out, fitness, rmse, nullptr, &tr);
}

extern "C" int alignnet_debug_icp_grid(alignnet_handle* h, const float* points1, int64_t n1, const float* points2, int64_t n2, const double* T,
                                       double radius, int32_t flags, int32_t* index, double* dist2, int32_t* inlier, int32_t* candidates,
                                       double* cell_edge, int32_t* buckets_occupied, int32_t* largest_bucket, double* fitness, double* rmse)
{
  const std::string name("alignnet_debug_icp_grid");
  bool full = false;
  int64_t off[4];
  if (debug_arguments(h, name, flags, n1, n2, &full, off)) return 1;
  if (!index || !dist2 || !inlier || !candidates || !cell_edge || !buckets_occupied || !largest_bucket) return fail(h, name + ": null output");
  IcpGridInfo info = {0.0, 0, 0, 0, 0};
  const IcpTraceOut tr = {n1, 0, index, dist2, inlier, candidates, nullptr, true, &info};
  double out[16];
  if (icp_host(h, name.c_str(), points1, points2, off, 1, T, radius, 0, full, out, fitness, rmse, nullptr, &tr)) return 1;
  *cell_edge = info.edge; *buckets_occupied = info.occupied; *largest_bucket = info.largest;
  return 0;
}

extern "C" int alignnet_icp_plane_register(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets, int32_t B,
                                           const double* init, double radius, double normal_radius, int32_t its, int32_t flags, double* out,
                                           double* fitness, double* rmse, int32_t* iterations)
{
  bool full = false;
  if (icp_flags(h, "alignnet_icp_plane_register", flags, &full)) return 1;
  return icp_plane_host(h, "alignnet_icp_plane_register", points1, points2, offsets, B, init, radius, normal_radius, its, full, false, out, fitness, rmse, iterations);
}

extern "C" int alignnet_icp_plane_register_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, const double* init, double radius,
                                                   double normal_radius, int32_t its, int32_t flags, double* out, double* fitness, double* rmse,
                                                   int32_t* iterations)
{
  const std::string name("alignnet_icp_plane_register_dataset");
  bool full = false;
  if (icp_flags(h, name, flags, &full)) return 1;
  IcpClouds c;
  if (stage_rows(h, name, rows, B, &c)) return 1;
  return run_icp_plane(h, c, B, init, radius, normal_radius, its, full, false, out, fitness, rmse, iterations);
}

extern "C" int alignnet_debug_icp_plane(alignnet_handle* h, const float* points1, int64_t n1, const float* points2, int64_t n2, const double* T,
                                        double radius, double normal_radius, int32_t flags, double* normals, int32_t* neighbours, int32_t* index,
                                        double* dist2, int32_t* inlier, double* residual, double* sums, double* update, double* fitness, double* rmse)
{
  const std::string name("alignnet_debug_icp_plane");
  bool full = false;
  int64_t off[4];
  if (debug_arguments(h, name, flags, n1, n2, &full, off)) return 1;
  if (!normals || !neighbours || !index || !dist2 || !inlier || !residual || !sums || !update) return fail(h, name + ": null output");
  double up[12];
  const IcpPlaneTrace tr = {n1, n2, normals, neighbours, index, dist2, inlier, residual, sums, up};
  double out[16];
  if (icp_plane_host(h, name.c_str(), points1, points2, off, 1, T, radius, normal_radius, 0, full, false, out, fitness, rmse, nullptr, &tr)) return 1;
  debug_update(up, n1 > 0 && n2 > 0, update);
  return 0;
}

extern "C" int alignnet_icp_generalized_register(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets, int32_t B,
                                                 const double* init, double radius, double normal_radius, int32_t its, int32_t flags, double* out,
                                                 double* fitness, double* rmse, int32_t* iterations)
{
  bool full = false;
  if (icp_flags(h, "alignnet_icp_generalized_register", flags, &full)) return 1;
  return icp_plane_host(h, "alignnet_icp_generalized_register", points1, points2, offsets, B, init, radius, normal_radius, its, full, true, out, fitness,
                        rmse, iterations);
}

extern "C" int alignnet_icp_generalized_register_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, const double* init, double radius,
                                                         double normal_radius, int32_t its, int32_t flags, double* out, double* fitness, double* rmse,
                                                         int32_t* iterations)
{
  const std::string name("alignnet_icp_generalized_register_dataset");
  bool full = false;
  if (icp_flags(h, name, flags, &full)) return 1;
  IcpClouds c;
  if (stage_rows(h, name, rows, B, &c)) return 1;
  return run_icp_plane(h, c, B, init, radius, normal_radius, its, full, true, out, fitness, rmse, iterations);
}

extern "C" int alignnet_debug_icp_generalized(alignnet_handle* h, const float* points1, int64_t n1, const float* points2, int64_t n2, const double* T,
                                              double radius, double normal_radius, int32_t flags, double* target_normals, int32_t* target_neighbours,
                                              double* source_normals, int32_t* source_neighbours, int32_t* index, double* dist2, int32_t* inlier,
                                              double* sums, double* update, double* fitness, double* rmse)
{
  const std::string name("alignnet_debug_icp_generalized");
  bool full = false;
  int64_t off[4];
  if (debug_arguments(h, name, flags, n1, n2, &full, off)) return 1;
  if (!target_normals || !target_neighbours || !source_normals || !source_neighbours || !index || !dist2 || !inlier || !sums || !update)
    return fail(h, name + ": null output");
  double up[12];
  IcpPlaneTrace tr = {n1, n2, target_normals, target_neighbours, index, dist2, inlier, nullptr, sums, up};
  tr.src_normals = source_normals; tr.src_neighbours = source_neighbours;
  double out[16];
  if (icp_plane_host(h, name.c_str(), points1, points2, off, 1, T, radius, normal_radius, 0, full, true, out, fitness, rmse, nullptr, &tr)) return 1;
  debug_update(up, n1 > 0 && n2 > 0, update);
  return 0;
}

extern "C" void alignnet_icp_free(alignnet_handle* h)
{
  if (!h || !h->icp_grid_ws) return;
  hipFree(h->icp_grid_ws);
  h->icp_grid_ws = nullptr; h->icp_grid_ws_bytes = h->icp_grid_ws_used = 0;
}
