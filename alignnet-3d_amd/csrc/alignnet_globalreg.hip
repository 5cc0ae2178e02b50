// Global registration of a pair of FULL clouds: RANSAC on FPFH feature matches (the reference's `o3_gicp` baseline, icp.py:85-143:
// voxel_down_sample(0.05) -> estimate_normals(hybrid 0.10 / 30) -> compute_fpfh_feature(hybrid 0.25 / 100) ->
// registration_ransac_based_on_feature_matching(ransac_n 4, threshold 0.075, edge-length 0.9 + distance checkers,
// RANSACConvergenceCriteria(4000000, 500))), gfx950 only.
//
// UNPINNED: Open3D is not part of the reference tree and is not available next to this stack.  The computation is DEFINED by the text
// restated in tests/global_reg_ref.py (Open3D's published algorithms of the 0.7 line), which these kernels follow stage by stage; two
// points are this project's own and make results statistically, not numerically, comparable with Open3D's: the output order of the
// downsample (ascending (ix, iy, iz)) and the counter-based random generator of the RANSAC draws (gr_draw below).
//
// Every decision (floor, radius tests, argmin, the RANSAC checks) is taken on fp64 values.  Stages, each a kernel over a chunk of pairs, the
// arrays between them in a workspace owned by the handle:
//   gr_voxel_kernel       one workgroup per cloud: voxel keys, a bitonic sort of (key, point) in HBM, segment heads, per-voxel means
//   gr_neighbours_kernel  one wave per downsampled point: the points within the radius (an x-slab of the sorted voxels is scanned), the
//                         max_nn nearest by rank selection where there are more
//   gr_normals_kernel     one lane per point: covariance of the neighbours, 3x3 Jacobi eigenvectors
//   gr_spfh_kernel / gr_fpfh_kernel   one wave per point
//   gr_match_kernel       one workgroup per pair: nearest target feature of every source feature (fp64, target tiles in LDS)
//   gr_grid_kernel        one workgroup per pair: a uniform grid (cell >= the RANSAC threshold) over the downsampled target, counting sort
//   gr_ransac_kernel      one workgroup per pair: 1024 iterations are drawn and pre-checked at once (one per lane); the lanes that pass are
//                         validated in iteration order by the whole workgroup against the grid (LDS-resident when it fits, else from HBM)
//                         until max_validation have been -- so "the first max_validation that pass, in iteration order" is what is
//                         validated, whatever the launch shape.
// Fast global registration (FGR, the reference's `o3_gicp_fast`, icp.py:121-143; DEFINED by tests/fgr_ref.py) shares stages 1-5 and the grid:
// section 8 below (gr_match_kernel<true>, fgr_tuple_kernel, fgr_optimise_kernel, fgr_score_kernel) and alignnet_fgr_register*.
#include "engine.h"
#include "host_util.h"
#include "icp_estimate.h"
#include <cmath>
#include <vector>

namespace {

constexpr int kThreads = 1024, kWaves = kThreads / 64;
constexpr double kVoxel = 0.05;
constexpr int kNbrStride = 100;            // neighbour list row: max_nn of the FPFH search (the normals' 30 use its head)
constexpr int kBins = 33;
constexpr int kMaxCells = 32768;           // cells of the validation grid (HBM path); the LDS path takes what fits beside the points
constexpr int kMinLdsCells = 512;
constexpr int kLdsBytes = 150 * 1024;      // dynamic LDS of gr_ransac_kernel<., true>
constexpr int kMatchTile = 128;
constexpr int kCandLds = 320;             // candidates per wave that the neighbour search keeps in LDS
constexpr double kPi = 3.14159265358979323846;

struct GrArgs {
  const float* pts[2];          // point blobs
  const long long* off;         // [n + 1][2] row offsets into the blobs
  const int* rows;              // [Bc] example rows of this chunk, or null: pair b is row pair0 + b
  const int* streams;           // [Bc] or null
  long long pair0;
  long long cap, P2;            // largest raw cloud of the chunk; sort stride (power of two >= cap)
  // per cloud c = 2 * pair + side
  unsigned long long* key; int* val; int* seg;
  double* dpts; int* vox; int* npts; int* m;
  double* nrm; int* nbr; int* nbrc;
  double* cd2; int* cidx;
  double* spfh; double* fpfh;
  // per pair
  int* match; int* cell; int* cellfill; double* gpts; double* gpar; int* gdim;
  int* rmatch;                  // FGR only: [pairs][cap] nearest source feature of every target feature
  int* err;
  // RANSAC
  unsigned long long seed; long long max_iteration; int max_validation;
  double* out_T; double* out_fit; double* out_rmse; long long* out_iters; int* out_vals; long long* out_win;
};

__device__ __forceinline__ void gr_cloud(const GrArgs& a, int c, const float** p, long long* n)
{
  const int bl = c >> 1, side = c & 1;
  const long long row = a.rows ? a.rows[bl] : a.pair0 + bl;
  const long long lo = a.off[row * 2 + side];
  *n = a.off[(row + 1) * 2 + side] - lo;
  *p = a.pts[side] + lo * 3;
}

// exclusive scan of one int per thread over the workgroup; *total = the sum.  sh: [kWaves + 1]
__device__ __forceinline__ int gr_block_scan(int v, int* sh, int* total)
{
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
  __syncthreads();
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  if (threadIdx.x == 0) { int s = 0; for (int i = 0; i < kWaves; ++i) { const int t = sh[i]; sh[i] = s; s += t; } sh[kWaves] = s; }
  __syncthreads();
  *total = sh[kWaves];
  return sh[w] + inc - v;
}

// ---- 1. voxel downsample -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gr_voxel_kernel(const GrArgs a)
{
  __shared__ float smin[3][kWaves];
  __shared__ int sh[kWaves + 1];
  const int c = blockIdx.x, tid = threadIdx.x;
  const float* p; long long nl;
  gr_cloud(a, c, &p, &nl);
  const int n = (int)nl;
  if (n == 0) { if (tid == 0) a.m[c] = 0; return; }
  unsigned long long* key = a.key + (size_t)c * a.P2;
  int* val = a.val + (size_t)c * a.P2;
  int* seg = a.seg + (size_t)c * (a.cap + 1);
  float mn[3] = {INFINITY, INFINITY, INFINITY};
  for (int i = tid; i < n; i += kThreads)
#pragma unroll
    for (int k = 0; k < 3; ++k) mn[k] = fminf(mn[k], p[(size_t)i * 3 + k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn[k] = fminf(mn[k], __shfl_xor(mn[k], o));
    if ((tid & 63) == 0) smin[k][tid >> 6] = mn[k];
  }
  __syncthreads();
  double m0[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float v = smin[k][0];
    for (int w = 1; w < kWaves; ++w) v = fminf(v, smin[k][w]);
    m0[k] = (double)v - kVoxel / 2.0;
  }
  int P = 1;
  while (P < n) P <<= 1;
  for (int i = tid; i < P; i += kThreads) {
    unsigned long long kk = ~0ull;
    if (i < n) {
      kk = 0;
      bool ok = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double f = floor(((double)p[(size_t)i * 3 + k] - m0[k]) / kVoxel);
        if (f >= 0.0 && f < 2097152.0) kk = (kk << 21) | (unsigned long long)(long long)f; else ok = false;
      }
      if (!ok) { kk = 0; *a.err = 1; }   // not finite, or a cloud wider than 2^21 voxels: reported by the host, never truncated
    }
    key[i] = kk; val[i] = i;
  }
  __syncthreads();
  // bitonic sort of (key, point index), ascending
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += kThreads) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long ki = key[i], kl = key[l];
          const int vi = val[i], vl = val[l];
          const bool gt = ki > kl || (ki == kl && vi > vl);
          if (gt == ((i & k) == 0)) { key[i] = kl; key[l] = ki; val[i] = vl; val[l] = vi; }
        }
      }
      __syncthreads();
    }
  // segment heads -> one output point per occupied voxel, in ascending key order
  const int per = (n + kThreads - 1) / kThreads;
  const int s0 = min(n, tid * per), s1 = min(n, s0 + per);
  int heads = 0;
  for (int i = s0; i < s1; ++i) heads += (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
  int m;
  int o = gr_block_scan(heads, sh, &m);
  for (int i = s0; i < s1; ++i)
    if (i == 0 || key[i] != key[i - 1]) seg[o++] = i;
  if (tid == 0) { seg[m] = n; a.m[c] = m; }
  __syncthreads();
  double* dp = a.dpts + (size_t)c * a.cap * 3;
  int* vx = a.vox + (size_t)c * a.cap * 3;
  int* np = a.npts + (size_t)c * a.cap;
  for (int q = tid; q < m; q += kThreads) {
    const int b = seg[q], e = seg[q + 1];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int i = b; i < e; ++i) {   // ascending point index
      const size_t s = (size_t)val[i] * 3;
      sx += (double)p[s]; sy += (double)p[s + 1]; sz += (double)p[s + 2];
    }
    const double cnt = (double)(e - b);
    dp[(size_t)q * 3] = sx / cnt; dp[(size_t)q * 3 + 1] = sy / cnt; dp[(size_t)q * 3 + 2] = sz / cnt;
    const unsigned long long kk = key[b];
    vx[(size_t)q * 3] = (int)(kk >> 42); vx[(size_t)q * 3 + 1] = (int)((kk >> 21) & 0x1fffff); vx[(size_t)q * 3 + 2] = (int)(kk & 0x1fffff);
    np[q] = e - b;
  }
}

// ---- 2. neighbours within a radius, the kMaxNN nearest where there are more -----------------------------------------------------------
__device__ __forceinline__ int gr_lower_bound_x(const int* vx, int m, int x)
{
  int lo = 0, hi = m;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (vx[(size_t)mid * 3] < x) lo = mid + 1; else hi = mid; }
  return lo;
}

template <int kMaxNN>
__global__ __launch_bounds__(kThreads) void gr_neighbours_kernel(const GrArgs a, const double radius, const int slabs)
{
  __shared__ double ld2[kWaves][kCandLds];   // the wave's candidates, for the rank selection (the HBM copy serves a wave with more)
  __shared__ int lidx[kWaves][kCandLds];
  const int c = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int m = a.m[c];
  const double* dp = a.dpts + (size_t)c * a.cap * 3;
  const int* vx = a.vox + (size_t)c * a.cap * 3;
  int* nbr = a.nbr + (size_t)c * a.cap * kNbrStride;
  int* nbrc = a.nbrc + (size_t)c * a.cap;
  double* cd2 = a.cd2 + ((size_t)c * kWaves + wave) * a.cap;
  int* cidx = a.cidx + ((size_t)c * kWaves + wave) * a.cap;
  const double r2 = radius * radius;
  // the downsampled points are sorted by ix first: everything within the radius lies in the slab |ix' - ix| <= slabs.  Its bounds are found
  // for all points at once, one lane per point (the searches are chains of dependent loads: 1024 of them in flight instead of one per wave),
  // into the voxel stage's sort arrays, which are free by now
  int* slo = a.seg + (size_t)c * (a.cap + 1);
  int* shi = a.val + (size_t)c * a.P2;
  for (int i = threadIdx.x; i < m; i += kThreads) {
    const int ix = vx[(size_t)i * 3];
    slo[i] = gr_lower_bound_x(vx, m, ix - slabs); shi[i] = gr_lower_bound_x(vx, m, ix + slabs + 1);
  }
  __syncthreads();
  for (int i = wave; i < m; i += kWaves) {
    const int lo = slo[i], hi = shi[i];
    const double px = dp[(size_t)i * 3], py = dp[(size_t)i * 3 + 1], pz = dp[(size_t)i * 3 + 2];
    int tot = 0;
    for (int j0 = lo; j0 < hi; j0 += 64) {
      const int j = j0 + lane;
      bool in = false; double d2 = 0.0;
      if (j < hi) {
        const double dx = dp[(size_t)j * 3] - px, dy = dp[(size_t)j * 3 + 1] - py, dz = dp[(size_t)j * 3 + 2] - pz;
        d2 = dx * dx + dy * dy + dz * dz;
        in = d2 <= r2;
      }
      const unsigned long long b = __ballot(in);
      if (in) {
        const int pos = tot + __popcll(b & ((1ull << lane) - 1ull));
        if (tot + __popcll(b) <= kMaxNN) nbr[(size_t)i * kNbrStride + pos] = j;   // while everything fits: ascending index
        cd2[pos] = d2; cidx[pos] = j;
        if (pos < kCandLds) { ld2[wave][pos] = d2; lidx[wave][pos] = j; }
      }
      tot += __popcll(b);
    }
    if (tot > kMaxNN) {   // more than max_nn within the radius: the max_nn smallest by (distance, index), in that order
      __threadfence_block();
      const bool in_lds = tot <= kCandLds;
      for (int q = lane; q < tot; q += 64) {
        const double dq = in_lds ? ld2[wave][q] : cd2[q]; const int iq = in_lds ? lidx[wave][q] : cidx[q];
        int rank = 0;
        if (in_lds) {
#pragma unroll 4
          for (int r = 0; r < tot; ++r) {
            const double dr = ld2[wave][r]; const int ir = lidx[wave][r];
            rank += (dr < dq || (dr == dq && ir < iq)) ? 1 : 0;
          }
        } else {
          for (int r = 0; r < tot; ++r) {
            const double dr = cd2[r]; const int ir = cidx[r];
            rank += (dr < dq || (dr == dq && ir < iq)) ? 1 : 0;
          }
        }
        if (rank < kMaxNN) nbr[(size_t)i * kNbrStride + rank] = iq;
      }
      __threadfence_block();
    }
    if (lane == 0) nbrc[i] = min(tot, kMaxNN);
  }
}

// ---- 3. normals (icp_estimate.h: icp_smallest_eigenvector) ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gr_normals_kernel(const GrArgs a)
{
  const int c = blockIdx.x;
  const int m = a.m[c];
  const double* dp = a.dpts + (size_t)c * a.cap * 3;
  const int* nbr = a.nbr + (size_t)c * a.cap * kNbrStride;
  const int* nbrc = a.nbrc + (size_t)c * a.cap;
  double* nrm = a.nrm + (size_t)c * a.cap * 3;
  for (int i = blockIdx.y * 256 + threadIdx.x; i < m; i += gridDim.y * 256) {
    const int K = nbrc[i];
    double n[3] = {0.0, 0.0, 1.0};
    if (K >= 3) {
      const int* row = nbr + (size_t)i * kNbrStride;
      double mx = 0.0, my = 0.0, mz = 0.0;
      for (int k = 0; k < K; ++k) { const size_t j = (size_t)row[k] * 3; mx += dp[j]; my += dp[j + 1]; mz += dp[j + 2]; }
      mx /= (double)K; my /= (double)K; mz /= (double)K;
      double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
      for (int k = 0; k < K; ++k) {
        const size_t j = (size_t)row[k] * 3;
        const double x = dp[j] - mx, y = dp[j + 1] - my, z = dp[j + 2] - mz;
        c00 += x * x; c01 += x * y; c02 += x * z; c11 += y * y; c12 += y * z; c22 += z * z;
      }
      const double inv = (double)K;
      icp_smallest_eigenvector(c00 / inv, c01 / inv, c02 / inv, c11 / inv, c12 / inv, c22 / inv, n);
      const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
      if (!(nn > 0.0)) { n[0] = 0.0; n[1] = 0.0; n[2] = 1.0; }
      else { n[0] /= nn; n[1] /= nn; n[2] /= nn; }
      if (n[2] < 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
    }
    nrm[(size_t)i * 3] = n[0]; nrm[(size_t)i * 3 + 1] = n[1]; nrm[(size_t)i * 3 + 2] = n[2];
  }
}

// ---- 4. SPFH / FPFH ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int gr_bin(double v)
{
  if (!(v >= 0.0)) return 0;
  return v >= 11.0 ? 10 : (int)floor(v);
}

// the three histogram bins of the pair feature of (p1, n1), (p2, n2)
__device__ __forceinline__ void gr_pair_bins(const double* p1, const double* n1, const double* p2, const double* n2, int* bins)
{
  double f0 = 0.0, f1 = 0.0, f2 = 0.0;
  double d[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  const double f3 = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (f3 != 0.0) {
    const double a1 = (n1[0] * d[0] + n1[1] * d[1] + n1[2] * d[2]) / f3;
    const double a2 = (n2[0] * d[0] + n2[1] * d[1] + n2[2] * d[2]) / f3;
    const double* n1c = n1; const double* n2c = n2;
    if (acos(fabs(a1)) > acos(fabs(a2))) { n1c = n2; n2c = n1; d[0] = -d[0]; d[1] = -d[1]; d[2] = -d[2]; f2 = -a2; }
    else f2 = a1;
    double v[3] = {d[1] * n1c[2] - d[2] * n1c[1], d[2] * n1c[0] - d[0] * n1c[2], d[0] * n1c[1] - d[1] * n1c[0]};
    const double vn = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (vn == 0.0) { f0 = 0.0; f1 = 0.0; f2 = 0.0; }
    else {
      v[0] /= vn; v[1] /= vn; v[2] /= vn;
      const double w[3] = {n1c[1] * v[2] - n1c[2] * v[1], n1c[2] * v[0] - n1c[0] * v[2], n1c[0] * v[1] - n1c[1] * v[0]};
      f1 = v[0] * n2c[0] + v[1] * n2c[1] + v[2] * n2c[2];
      f0 = atan2(w[0] * n2c[0] + w[1] * n2c[1] + w[2] * n2c[2], n1c[0] * n2c[0] + n1c[1] * n2c[1] + n1c[2] * n2c[2]);
    }
  }
  bins[0] = gr_bin(11.0 * (f0 + kPi) / (2.0 * kPi));
  bins[1] = 11 + gr_bin(11.0 * (f1 + 1.0) / 2.0);
  bins[2] = 22 + gr_bin(11.0 * (f2 + 1.0) / 2.0);
}

__global__ __launch_bounds__(kThreads) void gr_spfh_kernel(const GrArgs a)
{
  __shared__ int hist[kWaves][kBins];
  const int c = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int m = a.m[c];
  const double* dp = a.dpts + (size_t)c * a.cap * 3;
  const double* nrm = a.nrm + (size_t)c * a.cap * 3;
  const int* nbr = a.nbr + (size_t)c * a.cap * kNbrStride;
  const int* nbrc = a.nbrc + (size_t)c * a.cap;
  double* spfh = a.spfh + (size_t)c * a.cap * kBins;
  for (int i = blockIdx.y * kWaves + wave; i < m; i += gridDim.y * kWaves) {
    const int K = nbrc[i];
    if (lane < kBins) hist[wave][lane] = 0;
    __builtin_amdgcn_wave_barrier();
    if (K >= 2) {
      const double p1[3] = {dp[(size_t)i * 3], dp[(size_t)i * 3 + 1], dp[(size_t)i * 3 + 2]};
      const double n1[3] = {nrm[(size_t)i * 3], nrm[(size_t)i * 3 + 1], nrm[(size_t)i * 3 + 2]};
      for (int k = lane; k < K; k += 64) {
        const int j = nbr[(size_t)i * kNbrStride + k];
        if (j == i) continue;
        const double p2[3] = {dp[(size_t)j * 3], dp[(size_t)j * 3 + 1], dp[(size_t)j * 3 + 2]};
        const double n2[3] = {nrm[(size_t)j * 3], nrm[(size_t)j * 3 + 1], nrm[(size_t)j * 3 + 2]};
        int bins[3];
        gr_pair_bins(p1, n1, p2, n2, bins);
        atomicAdd(&hist[wave][bins[0]], 1); atomicAdd(&hist[wave][bins[1]], 1); atomicAdd(&hist[wave][bins[2]], 1);
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (lane < kBins) spfh[(size_t)i * kBins + lane] = K >= 2 ? (double)hist[wave][lane] * (100.0 / (double)(K - 1)) : 0.0;
    __builtin_amdgcn_wave_barrier();
  }
}

__global__ __launch_bounds__(kThreads) void gr_fpfh_kernel(const GrArgs a)
{
  __shared__ double acc[kWaves][kBins];
  __shared__ double wD[kWaves][kNbrStride];
  __shared__ int wJ[kWaves][kNbrStride];
  const int c = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int m = a.m[c];
  const double* dp = a.dpts + (size_t)c * a.cap * 3;
  const int* nbr = a.nbr + (size_t)c * a.cap * kNbrStride;
  const int* nbrc = a.nbrc + (size_t)c * a.cap;
  const double* spfh = a.spfh + (size_t)c * a.cap * kBins;
  double* fpfh = a.fpfh + (size_t)c * a.cap * kBins;
  for (int i = blockIdx.y * kWaves + wave; i < m; i += gridDim.y * kWaves) {
    const int K = nbrc[i];
    const double px = dp[(size_t)i * 3], py = dp[(size_t)i * 3 + 1], pz = dp[(size_t)i * 3 + 2];
    // the neighbours' indices and squared distances first, a lane per neighbour (0 marks the point itself: skipped like any D = 0)
    for (int k = lane; k < K; k += 64) {
      const int j = nbr[(size_t)i * kNbrStride + k];
      const double dx = dp[(size_t)j * 3] - px, dy = dp[(size_t)j * 3 + 1] - py, dz = dp[(size_t)j * 3 + 2] - pz;
      wJ[wave][k] = j; wD[wave][k] = j == i ? 0.0 : dx * dx + dy * dy + dz * dz;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    double s = 0.0;
    if (lane < kBins && K >= 2) {
#pragma unroll 4
      for (int k = 0; k < K; ++k) {   // list order: ascending index, or ascending (distance, index) where max_nn cut the set
        const double D = wD[wave][k];
        if (D > 0.0) s += spfh[(size_t)wJ[wave][k] * kBins + lane] / D;
      }
    }
    if (lane < kBins) acc[wave][lane] = s;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (lane < kBins) {
      const int g = lane / 11;
      double gs = 0.0;
      for (int q = 0; q < 11; ++q) gs += acc[wave][g * 11 + q];
      if (gs != 0.0) s *= 100.0 / gs;
      fpfh[(size_t)i * kBins + lane] = s + spfh[(size_t)i * kBins + lane];
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- 5. feature matches: for every source feature the nearest target feature (lowest index wins a tie) --------------------------------
// kReverse (FGR): the roles swapped -- for every target feature the nearest source feature, into a.rmatch
template <bool kReverse>
__global__ __launch_bounds__(kThreads) void gr_match_kernel(const GrArgs a)
{
  __shared__ double tile[kMatchTile][kBins];
  const int bl = blockIdx.x, tid = threadIdx.x;
  const int ms = a.m[2 * bl + (kReverse ? 1 : 0)], mt = a.m[2 * bl + (kReverse ? 0 : 1)];
  const double* fs = a.fpfh + (size_t)(2 * bl + (kReverse ? 1 : 0)) * a.cap * kBins;
  const double* ft = a.fpfh + (size_t)(2 * bl + (kReverse ? 0 : 1)) * a.cap * kBins;
  int* match = (kReverse ? a.rmatch : a.match) + (size_t)bl * a.cap;
  for (int i0 = 0; i0 < ms; i0 += kThreads) {
    const int i = i0 + tid;
    const bool active = i < ms;
    double f[kBins];
#pragma unroll
    for (int k = 0; k < kBins; ++k) f[k] = active ? fs[(size_t)i * kBins + k] : 0.0;
    double best = INFINITY; int bj = 0;
    for (int t0 = 0; t0 < mt; t0 += kMatchTile) {
      const int nt = min(kMatchTile, mt - t0);
      __syncthreads();
      for (int q = tid; q < nt * kBins; q += kThreads) (&tile[0][0])[q] = ft[(size_t)t0 * kBins + q];
      __syncthreads();
      for (int t = 0; t < nt; ++t) {
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < kBins; ++k) { const double e = f[k] - tile[t][k]; d += e * e; }
        if (d < best) { best = d; bj = t0 + t; }
      }
    }
    if (active) match[i] = bj;
  }
}

// cell of coordinate x along an axis of n cells (clamped: a point on the upper face, or a coordinate that is not finite)
__device__ __forceinline__ int gr_cell(double x, double mn, double cs, int n)
{
  const double f = floor((x - mn) / cs);
  return f >= 0.0 ? (f < (double)n ? (int)f : n - 1) : 0;
}

// ---- 6. the validation grid over the downsampled target ------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gr_grid_kernel(const GrArgs a, const double tau)
{
  __shared__ double red[6][kWaves];
  __shared__ double par[4];
  __shared__ int dim[4];
  __shared__ int sh[kWaves + 1];
  const int bl = blockIdx.x, tid = threadIdx.x;
  const int mt = a.m[2 * bl + 1];
  const double* tp = a.dpts + (size_t)(2 * bl + 1) * a.cap * 3;
  int* cell = a.cell + (size_t)bl * (kMaxCells + 1);
  int* fill = a.cellfill + (size_t)bl * kMaxCells;
  double* gx = a.gpts + (size_t)bl * a.cap * 3; double* gy = gx + a.cap; double* gz = gy + a.cap;
  double v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int j = tid; j < mt; j += kThreads)
#pragma unroll
    for (int k = 0; k < 3; ++k) { const double x = tp[(size_t)j * 3 + k]; v[k] = fmin(v[k], x); v[3 + k] = fmax(v[3 + k], x); }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_xor(v[k], o); v[k] = k < 3 ? fmin(v[k], t) : fmax(v[k], t); }
    if ((tid & 63) == 0) red[k][tid >> 6] = v[k];
  }
  __syncthreads();
  if (tid == 0) {
    double e[6];
    for (int k = 0; k < 6; ++k) { e[k] = red[k][0]; for (int w = 1; w < kWaves; ++w) e[k] = k < 3 ? fmin(e[k], red[k][w]) : fmax(e[k], red[k][w]); }
    const long long lds_cells = ((long long)kLdsBytes - 24ll * mt) / 4 - 2;
    const int use_lds = lds_cells >= kMinLdsCells ? 1 : 0;
    const long long cells_cap = use_lds ? (lds_cells < kMaxCells ? lds_cells : (long long)kMaxCells) : (long long)kMaxCells;
    double cs = 1.001 * tau;
    int nx = 1, ny = 1, nz = 1;
    if (mt > 0) {
      bool found = false;
      for (int g = 0; g < 400 && !found; ++g) {   // 1.1^400 covers every extent the voxel stage accepts
        const double fx = floor((e[3] - e[0]) / cs), fy = floor((e[4] - e[1]) / cs), fz = floor((e[5] - e[2]) / cs);
        if (fx >= 0.0 && fy >= 0.0 && fz >= 0.0 && fx < 40000.0 && fy < 40000.0 && fz < 40000.0) {
          nx = (int)fx + 1; ny = (int)fy + 1; nz = (int)fz + 1;
          found = (long long)nx * ny * nz <= cells_cap;
        }
        if (!found) cs *= 1.1;
      }
      if (!found) { nx = 1; ny = 1; nz = 1; }   // not finite (reported through a.err): one cell
    }
    par[0] = mt > 0 ? e[0] : 0.0; par[1] = mt > 0 ? e[1] : 0.0; par[2] = mt > 0 ? e[2] : 0.0; par[3] = cs;
    dim[0] = nx; dim[1] = ny; dim[2] = nz; dim[3] = use_lds;
    for (int k = 0; k < 4; ++k) { a.gpar[(size_t)bl * 4 + k] = par[k]; a.gdim[(size_t)bl * 4 + k] = dim[k]; }
  }
  __syncthreads();
  const int nx = dim[0], ny = dim[1], nz = dim[2], nc = dim[0] * dim[1] * dim[2];
  for (int q = tid; q < nc; q += kThreads) fill[q] = 0;
  __syncthreads();
  for (int j = tid; j < mt; j += kThreads) {
    const int cx = gr_cell(tp[(size_t)j * 3], par[0], par[3], nx), cy = gr_cell(tp[(size_t)j * 3 + 1], par[1], par[3], ny),
              cz = gr_cell(tp[(size_t)j * 3 + 2], par[2], par[3], nz);
    atomicAdd(&fill[(cz * ny + cy) * nx + cx], 1);
  }
  __syncthreads();
  const int per = (nc + kThreads - 1) / kThreads;
  const int s0 = min(nc, tid * per), s1 = min(nc, s0 + per);
  int cnt = 0;
  for (int q = s0; q < s1; ++q) cnt += fill[q];
  int total;
  int o = gr_block_scan(cnt, sh, &total);
  for (int q = s0; q < s1; ++q) { const int t = fill[q]; cell[q] = o; fill[q] = o; o += t; }
  if (tid == 0) cell[nc] = mt;
  __syncthreads();
  for (int j = tid; j < mt; j += kThreads) {
    const double x = tp[(size_t)j * 3], y = tp[(size_t)j * 3 + 1], z = tp[(size_t)j * 3 + 2];
    const int cx = gr_cell(x, par[0], par[3], nx), cy = gr_cell(y, par[1], par[3], ny), cz = gr_cell(z, par[2], par[3], nz);
    const int pos = atomicAdd(&fill[(cz * ny + cy) * nx + cx], 1);   // the order inside a cell is free: only the smallest distance is used
    gx[pos] = x; gy[pos] = y; gz[pos] = z;
  }
}

// ---- 7. RANSAC -----------------------------------------------------------------------------------------------------------------------
// draw k of iteration it: index into the n downsampled source points (counter-based: splitmix64's finaliser over seed, stream, it, k)
__device__ __forceinline__ int gr_draw(unsigned long long seed, unsigned long long stream, unsigned long long it, int k, int n)
{
  unsigned long long x = seed * 0x9E3779B97F4A7C15ull + ((stream << 40) | (it << 2) | (unsigned long long)k);
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull;
  const unsigned long long z = x ^ (x >> 31);
  return (int)(((z >> 32) * (unsigned long long)n) >> 32);
}

// one iteration: draw, edge-length check, estimate, distance check.  true = the hypothesis T (rows 0..2 of the 4x4) is to be validated
template <bool kFull>
__device__ __forceinline__ bool gr_hypothesis(unsigned long long seed, unsigned long long stream, unsigned long long it, int ms,
                                              const double* sp, const double* tp, const int* match, double tau2, double* T)
{
  double s[4][3], t[4][3];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = gr_draw(seed, stream, it, k, ms);
    const int j = match[i];
#pragma unroll
    for (int q = 0; q < 3; ++q) { s[k][q] = sp[(size_t)i * 3 + q]; t[k][q] = tp[(size_t)j * 3 + q]; }
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = j + 1; k < 4; ++k) {
      const double ax = s[j][0] - s[k][0], ay = s[j][1] - s[k][1], az = s[j][2] - s[k][2];
      const double bx = t[j][0] - t[k][0], by = t[j][1] - t[k][1], bz = t[j][2] - t[k][2];
      const double la = sqrt(ax * ax + ay * ay + az * az), lb = sqrt(bx * bx + by * by + bz * bz);
      if (la < 0.9 * lb || lb < 0.9 * la) ok = false;
    }
  if (!ok) return false;
  // the estimate of alignnet_icp.hip on these four correspondences: sums about a pivot (the first target point), then its closed forms
  const double cx = t[0][0], cy = t[0][1], cz = t[0][2], cnt = 4.0;
  double sa[3] = {0.0, 0.0, 0.0}, sb[3] = {0.0, 0.0, 0.0};
  double A[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double sxx = 0.0, sxy = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double ax = s[k][0] - cx, ay = s[k][1] - cy, az = s[k][2] - cz, bx = t[k][0] - cx, by = t[k][1] - cy, bz = t[k][2] - cz;
    sa[0] += ax; sa[1] += ay; sa[2] += az; sb[0] += bx; sb[1] += by; sb[2] += bz;
    if constexpr (kFull) {
      A[0] += bx * ax; A[1] += bx * ay; A[2] += bx * az; A[3] += by * ax; A[4] += by * ay; A[5] += by * az; A[6] += bz * ax; A[7] += bz * ay; A[8] += bz * az;
    } else {
      sxx += ax * bx + ay * by; sxy += ax * by - ay * bx;
    }
  }
  const double am[3] = {sa[0] / cnt, sa[1] / cnt, sa[2] / cnt}, bm[3] = {sb[0] / cnt, sb[1] / cnt, sb[2] / cnt};
  if constexpr (kFull) {
    double work[27];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) work[i * 3 + j] = A[i * 3 + j] - cnt * (bm[i] * am[j]);
    icp_umeyama_rotation(work);
    const double* R = work + 18;
    const double mp[3] = {cx + am[0], cy + am[1], cz + am[2]}, mq[3] = {cx + bm[0], cy + bm[1], cz + bm[2]};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      T[r * 4] = R[r * 3]; T[r * 4 + 1] = R[r * 3 + 1]; T[r * 4 + 2] = R[r * 3 + 2];
      T[r * 4 + 3] = mq[r] - (R[r * 3] * mp[0] + R[r * 3 + 1] * mp[1] + R[r * 3 + 2] * mp[2]);
    }
  } else {
    const double cxx = sxx - cnt * (am[0] * bm[0] + am[1] * bm[1]);
    const double cxy = sxy - cnt * (am[0] * bm[1] - am[1] * bm[0]);
    const double th = atan2(cxy, cxx), c = cos(th), sn = sin(th);
    const double mpx = cx + am[0], mpy = cy + am[1], mqx = cx + bm[0], mqy = cy + bm[1];
    T[0] = c; T[1] = -sn; T[2] = 0.0; T[3] = mqx - (c * mpx - sn * mpy);
    T[4] = sn; T[5] = c; T[6] = 0.0; T[7] = mqy - (sn * mpx + c * mpy);
    T[8] = 0.0; T[9] = 0.0; T[10] = 1.0; T[11] = bm[2] - am[2];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double dx = T[0] * s[k][0] + T[1] * s[k][1] + T[2] * s[k][2] + T[3] - t[k][0];
    const double dy = T[4] * s[k][0] + T[5] * s[k][1] + T[6] * s[k][2] + T[7] - t[k][1];
    const double dz = T[8] * s[k][0] + T[9] * s[k][1] + T[10] * s[k][2] + T[11] - t[k][2];
    if (dx * dx + dy * dy + dz * dz > tau2) ok = false;
  }
  return ok;
}

template <bool kFull, bool kLds>
__global__ __launch_bounds__(kThreads) void gr_ransac_kernel(const GrArgs a, const double tau)
{
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ unsigned long long wmask[kWaves];
  __shared__ double Tcur[12];
  __shared__ double red[kWaves * 2], tot[2];
  const int bl = blockIdx.x, tid = threadIdx.x;
  const int* gdim = a.gdim + (size_t)bl * 4;
  if ((gdim[3] != 0) != kLds) return;   // the other instantiation's pair
  const int ms = a.m[2 * bl], mt = a.m[2 * bl + 1];
  const double* sp = a.dpts + (size_t)(2 * bl) * a.cap * 3;
  const double* tp = a.dpts + (size_t)(2 * bl + 1) * a.cap * 3;
  const int* match = a.match + (size_t)bl * a.cap;
  const int nx = gdim[0], ny = gdim[1], nz = gdim[2], nc = nx * ny * nz;
  const double mnx = a.gpar[(size_t)bl * 4], mny = a.gpar[(size_t)bl * 4 + 1], mnz = a.gpar[(size_t)bl * 4 + 2], cs = a.gpar[(size_t)bl * 4 + 3];
  const double* gx; const double* gy; const double* gz; const int* cell;
  {
    const double* hx = a.gpts + (size_t)bl * a.cap * 3;
    const int* hc = a.cell + (size_t)bl * (kMaxCells + 1);
    if constexpr (kLds) {
      double* lx = lds; double* ly = lx + mt; double* lz = ly + mt;
      int* lc = reinterpret_cast<int*>(lz + mt);
      for (int j = tid; j < mt; j += kThreads) { lx[j] = hx[j]; ly[j] = hx[a.cap + j]; lz[j] = hx[2 * a.cap + j]; }
      for (int q = tid; q <= nc; q += kThreads) lc[q] = hc[q];
      gx = lx; gy = ly; gz = lz; cell = lc;
    } else {
      gx = hx; gy = hx + a.cap; gz = hx + 2 * a.cap; cell = hc;
    }
  }
  __syncthreads();
  const unsigned long long stream = a.streams ? (unsigned long long)a.streams[bl] : 0ull;
  const double tau2 = tau * tau;
  double bestT[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  double best_cnt = 0.0, best_rmse = 0.0;
  long long win = -1, iterations = 0;
  int validated = 0;
  if (ms >= 4 && mt >= 4 && a.max_validation > 0) {
    bool done = false;
    iterations = a.max_iteration;
    for (long long it0 = 0; it0 < a.max_iteration && !done; it0 += kThreads) {
      const long long it = it0 + tid;
      double T[12];
      const bool pass = it < a.max_iteration && gr_hypothesis<kFull>(a.seed, stream, (unsigned long long)it, ms, sp, tp, match, tau2, T);
      const unsigned long long bal = __ballot(pass);
      if ((tid & 63) == 0) wmask[tid >> 6] = bal;
      __syncthreads();
      for (int w = 0; w < kWaves && !done; ++w) {
        unsigned long long mk = wmask[w];
        while (mk != 0ull && !done) {
          const int l = __ffsll((unsigned long long)mk) - 1;
          mk &= mk - 1ull;
          const int tpass = w * 64 + l;
          if (tid == tpass)
#pragma unroll
            for (int q = 0; q < 12; ++q) Tcur[q] = T[q];
          __syncthreads();
          double Tl[12];
#pragma unroll
          for (int q = 0; q < 12; ++q) Tl[q] = Tcur[q];
          // ---- validate: nearest downsampled target point of every transformed downsampled source point, within tau ----
          double v[2] = {0.0, 0.0};
          for (int i = tid; i < ms; i += kThreads) {
            const double sx = sp[(size_t)i * 3], sy = sp[(size_t)i * 3 + 1], sz = sp[(size_t)i * 3 + 2];
            const double qx = Tl[0] * sx + Tl[1] * sy + Tl[2] * sz + Tl[3];
            const double qy = Tl[4] * sx + Tl[5] * sy + Tl[6] * sz + Tl[7];
            const double qz = Tl[8] * sx + Tl[9] * sy + Tl[10] * sz + Tl[11];
            const double fx = floor((qx - mnx) / cs), fy = floor((qy - mny) / cs), fz = floor((qz - mnz) / cs);
            if (!(fx >= -1.0 && fx <= (double)nx && fy >= -1.0 && fy <= (double)ny && fz >= -1.0 && fz <= (double)nz)) continue;
            const int x0 = max(0, (int)fx - 1), x1 = min(nx - 1, (int)fx + 1);
            const int y0 = max(0, (int)fy - 1), y1 = min(ny - 1, (int)fy + 1);
            const int z0 = max(0, (int)fz - 1), z1 = min(nz - 1, (int)fz + 1);
            if (x0 > x1) continue;
            double best = INFINITY;
            for (int z = z0; z <= z1; ++z)
              for (int y = y0; y <= y1; ++y) {
                const int rowc = (z * ny + y) * nx;
                const int b = cell[rowc + x0], e = cell[rowc + x1 + 1];   // cells along x are contiguous: one range per (y, z)
                for (int j = b; j < e; ++j) {
                  const double dx = qx - gx[j], dy = qy - gy[j], dz = qz - gz[j];
                  best = fmin(best, dx * dx + dy * dy + dz * dz);
                }
              }
            if (best <= tau2) { v[0] += 1.0; v[1] += best; }
          }
          // fixed-order sums: the result does not depend on anything but the pair
#pragma unroll
          for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
          if ((tid & 63) == 0) { red[(tid >> 6) * 2] = v[0]; red[(tid >> 6) * 2 + 1] = v[1]; }
          __syncthreads();
          if (tid < 2) { double sum = 0.0; for (int q = 0; q < kWaves; ++q) sum += red[q * 2 + tid]; tot[tid] = sum; }
          __syncthreads();
          const double cnt = tot[0];
          const double rmse = cnt > 0.0 ? sqrt(tot[1] / cnt) : 0.0;
          if (cnt > best_cnt || (cnt == best_cnt && rmse < best_rmse)) {
            best_cnt = cnt; best_rmse = rmse; win = it0 + tpass;
#pragma unroll
            for (int q = 0; q < 12; ++q) bestT[q] = Tl[q];
          }
          if (++validated == a.max_validation) { done = true; iterations = it0 + tpass + 1; }
        }
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
    const size_t b = (size_t)bl;
    for (int q = 0; q < 12; ++q) a.out_T[b * 16 + q] = bestT[q];
    a.out_T[b * 16 + 12] = 0.0; a.out_T[b * 16 + 13] = 0.0; a.out_T[b * 16 + 14] = 0.0; a.out_T[b * 16 + 15] = 1.0;
    a.out_fit[b] = ms > 0 ? best_cnt / (double)ms : 0.0;
    a.out_rmse[b] = best_rmse;
    a.out_iters[b] = iterations; a.out_vals[b] = validated; a.out_win[b] = win;
  }
}

// ---- 8. fast global registration (FGR, the reference's `o3_gicp_fast`; DEFINED by tests/fgr_ref.py) --------------------------------------
// On top of stages 1-5: the reverse matches (gr_match_kernel<true>), then per pair
//   fgr_tuple_kernel      one workgroup: the clouds' means and the normalising scale, the normalised points, the cross check (mutual matches
//                         compacted in ascending source index by block scans), then rounds of one tuple trial per lane; the lanes that pass
//                         are taken in trial order by ballot until max_tuples have been or ncorr * 100 trials are drawn
//   fgr_optimise_kernel   one workgroup: all Gauss-Newton iterations in one launch.  Per iteration each lane accumulates its correspondences'
//                         contributions to the 16 (full) / 8 (z-constrained) distinct sums of J^T J and J^T r, reduced in a fixed order
//                         (wave butterfly, then the waves in index order); every lane then solves the 6x6 / 4x4 system itself (Cholesky, fp64):
//                         the same instruction stream on the same sums, so no broadcast and one barrier per iteration.  The correspondences'
//                         points are gathered once into LDS (structure of arrays) when 3 max_tuples of them fit (up to 1024 tuples: Open3D's
//                         1000 does), else read through the index lists from HBM every iteration: the same arithmetic either way
//   gr_grid_kernel + fgr_score_kernel   fitness and inlier rmse of the result, threshold maximum_correspondence_distance
constexpr int kOptThreads = 512, kOptWaves = kOptThreads / 64;
constexpr int kOptLdsCorr = 3072;          // correspondences whose points fgr_optimise_kernel<., true> holds in LDS (48 bytes each)
constexpr int kFgrMinCorr = 10;
constexpr double kFgrPivotEps = 1e-12;

struct FgrArgs {
  double* npts;                 // [2 pairs][cap][3] normalised points
  double* norm;                 // [pairs][8]: mean of the source (3), of the target (3), scale
  int* cross; int* counts;      // [pairs][cap] cross-checked source indices; [pairs][2] their number, accepted tuples
  int* ci; int* cj;             // [pairs][3 max_tuples] tuple correspondences (source, target index)
  long long* ctrial;            // [pairs][max_tuples] trial index of every accepted tuple
  long long* trials;            // [pairs] trials drawn
  double* trace;                // [pairs][iterations][16] transform after every iteration (normalised frame), or null
  unsigned long long seed;
  double division_factor, max_corr_dist, tuple_scale;
  int iterations, max_tuples, decrease_mu;
};

__global__ __launch_bounds__(kThreads) void fgr_tuple_kernel(const GrArgs a, const FgrArgs f)
{
  __shared__ double red[kWaves][3];
  __shared__ double mean[2][3];
  __shared__ double s_scale;
  __shared__ int sh[kWaves + 1];
  __shared__ unsigned long long wmask[kWaves];
  __shared__ long long s_trials;
  const int bl = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ms = a.m[2 * bl], mt = a.m[2 * bl + 1];
  double* norm = f.norm + (size_t)bl * 8;
  int* counts = f.counts + (size_t)bl * 2;
  if (ms == 0 || mt == 0) {   // an empty cloud: nothing to normalise or to match
    if (tid < 8) norm[tid] = 0.0;
    if (tid == 0) { counts[0] = 0; counts[1] = 0; f.trials[bl] = 0; }
    return;
  }
  // ---- means, scale, normalised points ----
  double d2max = 0.0;
  for (int side = 0; side < 2; ++side) {
    const int m = side ? mt : ms;
    const double* dp = a.dpts + (size_t)(2 * bl + side) * a.cap * 3;
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < m; i += kThreads)
#pragma unroll
      for (int k = 0; k < 3; ++k) s[k] += dp[(size_t)i * 3 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o);
      if (lane == 0) red[w][k] = s[k];
    }
    __syncthreads();
    if (tid < 3) { double t = 0.0; for (int q = 0; q < kWaves; ++q) t += red[q][tid]; mean[side][tid] = t / (double)m; }
    __syncthreads();
    for (int i = tid; i < m; i += kThreads) {
      const double x = dp[(size_t)i * 3] - mean[side][0], y = dp[(size_t)i * 3 + 1] - mean[side][1], z = dp[(size_t)i * 3 + 2] - mean[side][2];
      d2max = fmax(d2max, x * x + y * y + z * z);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) d2max = fmax(d2max, __shfl_xor(d2max, o));
  if (lane == 0) red[w][0] = d2max;
  __syncthreads();
  if (tid == 0) { double t = 0.0; for (int q = 0; q < kWaves; ++q) t = fmax(t, red[q][0]); s_scale = sqrt(t); }
  __syncthreads();
  const double scale = s_scale;
  if (tid < 6) norm[tid] = mean[tid / 3][tid % 3];
  if (tid == 6) norm[6] = scale;
  if (tid == 7) norm[7] = 0.0;
  for (int side = 0; side < 2; ++side) {
    const int m = side ? mt : ms;
    const double* dp = a.dpts + (size_t)(2 * bl + side) * a.cap * 3;
    double* np = f.npts + (size_t)(2 * bl + side) * a.cap * 3;
    for (size_t q = tid; q < (size_t)m * 3; q += kThreads) np[q] = (dp[q] - mean[side][q % 3]) / scale;
  }
  // ---- cross check: the source indices whose match points back, ascending ----
  const int* match = a.match + (size_t)bl * a.cap;
  const int* rmatch = a.rmatch + (size_t)bl * a.cap;
  int* cross = f.cross + (size_t)bl * a.cap;
  int ncorr = 0;
  for (int i0 = 0; i0 < ms; i0 += kThreads) {
    const int i = i0 + tid;
    const int keep = (i < ms && rmatch[match[i]] == i) ? 1 : 0;
    int total;
    const int pos = gr_block_scan(keep, sh, &total);
    if (keep) cross[ncorr + pos] = i;
    ncorr += total;
  }
  if (tid == 0) { counts[0] = ncorr; s_trials = f.max_tuples > 0 ? (long long)ncorr * 100 : 0; }
  __syncthreads();   // the list and the normalised points are read back below
  // ---- tuple test ----
  const double* sp = f.npts + (size_t)(2 * bl) * a.cap * 3;
  const double* tp = f.npts + (size_t)(2 * bl + 1) * a.cap * 3;
  int* ci = f.ci + (size_t)bl * 3 * f.max_tuples;
  int* cj = f.cj + (size_t)bl * 3 * f.max_tuples;
  long long* ctrial = f.ctrial + (size_t)bl * f.max_tuples;
  const unsigned long long stream = a.streams ? (unsigned long long)a.streams[bl] : 0ull;
  const long long total = f.max_tuples > 0 ? (long long)ncorr * 100 : 0;
  const double ts = f.tuple_scale;
  int accepted = 0;
  for (long long t0 = 0; t0 < total && accepted < f.max_tuples; t0 += kThreads) {
    const long long t = t0 + tid;
    bool pass = false;
    int ii[3] = {0, 0, 0}, jj[3] = {0, 0, 0};
    if (t < total) {
      double p[3][3], q[3][3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        ii[k] = cross[gr_draw(f.seed, stream, (unsigned long long)t, k, ncorr)];
        jj[k] = match[ii[k]];
#pragma unroll
        for (int c = 0; c < 3; ++c) { p[k][c] = sp[(size_t)ii[k] * 3 + c]; q[k][c] = tp[(size_t)jj[k] * 3 + c]; }
      }
      pass = true;
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const int u = e, v = e == 2 ? 0 : e + 1;
        const double ax = p[v][0] - p[u][0], ay = p[v][1] - p[u][1], az = p[v][2] - p[u][2];
        const double bx = q[v][0] - q[u][0], by = q[v][1] - q[u][1], bz = q[v][2] - q[u][2];
        const double li = sqrt(ax * ax + ay * ay + az * az), lj = sqrt(bx * bx + by * by + bz * bz);
        if (!(li * ts < lj && lj < li / ts)) pass = false;
      }
    }
    const unsigned long long bal = __ballot(pass);
    if (lane == 0) wmask[w] = bal;
    __syncthreads();
    int before = 0, all = 0;
    for (int q = 0; q < kWaves; ++q) { const int c = __popcll(wmask[q]); before += q < w ? c : 0; all += c; }
    if (pass) {   // trial order = lane order
      const int pos = accepted + before + __popcll(bal & ((1ull << lane) - 1ull));
      if (pos < f.max_tuples) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { ci[(size_t)pos * 3 + k] = ii[k]; cj[(size_t)pos * 3 + k] = jj[k]; }
        ctrial[pos] = t;
        if (pos == f.max_tuples - 1) s_trials = t + 1;
      }
    }
    accepted = min(accepted + all, f.max_tuples);
    __syncthreads();
  }
  if (tid == 0) { counts[1] = accepted; f.trials[bl] = s_trials; }
}

// x with A x = b for the symmetric positive definite A (lower triangle used), Cholesky in index order.  false: a pivot is not greater than
// kFgrPivotEps times its diagonal entry.  One reciprocal per column (kept on the diagonal) instead of a division per entry: the solve is on
// the critical path of every iteration
template <int N>
__device__ __forceinline__ bool fgr_cholesky_solve(double (&A)[N][N], const double (&b)[N], double (&x)[N])
{
  bool ok = true;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double d = A[k][k];
#pragma unroll
    for (int j = 0; j < k; ++j) d -= A[k][j] * A[k][j];
    if (!(d > kFgrPivotEps * A[k][k])) { ok = false; d = 1.0; }
    const double il = 1.0 / sqrt(d);
    A[k][k] = il;
#pragma unroll
    for (int i = k + 1; i < N; ++i) {
      double v = A[i][k];
#pragma unroll
      for (int j = 0; j < k; ++j) v -= A[i][j] * A[k][j];
      A[i][k] = v * il;
    }
  }
  double y[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double v = b[i];
#pragma unroll
    for (int j = 0; j < i; ++j) v -= A[i][j] * y[j];
    y[i] = v * A[i][i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double v = y[i];
#pragma unroll
    for (int j = i + 1; j < N; ++j) v -= A[j][i] * x[j];
    x[i] = v * A[i][i];
  }
  return ok;
}

template <bool kFull, bool kLds>
__global__ __launch_bounds__(kOptThreads) void fgr_optimise_kernel(const GrArgs a, const FgrArgs f)
{
  extern __shared__ __attribute__((aligned(16))) double lds[];   // kLds: p_x p_y p_z q0_x q0_y q0_z, [n] each
  // the distinct sums: full  0..5 A00 A01 A02 A11 A12 A22 (rotation block), 6..8 sum s q, 9 sum s, 10..12 rotation part of J^T r, 13..15 sum s r
  //                    z-constrained  0 A22, 1..2 sum s q_x, s q_y, 3 sum s, 4 the z-rotation entry of J^T r, 5..7 sum s r
  constexpr int kSums = kFull ? 16 : 8;
  __shared__ double red[2][kOptWaves][kSums];
  const int bl = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ms = a.m[2 * bl], mt = a.m[2 * bl + 1];
  const int n = (ms == 0 || mt == 0) ? 0 : 3 * f.counts[(size_t)bl * 2 + 1];
  const double* sp = f.npts + (size_t)(2 * bl) * a.cap * 3;
  const double* tp = f.npts + (size_t)(2 * bl + 1) * a.cap * 3;
  const int* ci = f.ci + (size_t)bl * 3 * f.max_tuples;
  const int* cj = f.cj + (size_t)bl * 3 * f.max_tuples;
  double T[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  bool stopped = n < kFgrMinCorr;
  double mu = 1.0;
  if constexpr (kLds) {
    for (int c = tid; c < n; c += kOptThreads) {
      const size_t i = (size_t)ci[c] * 3, j = (size_t)cj[c] * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) { lds[k * n + c] = sp[i + k]; lds[(3 + k) * n + c] = tp[j + k]; }
    }
    __syncthreads();
  }
  for (int it = 0; it < f.iterations; ++it) {
    if (!stopped) {   // uniform over the workgroup: every lane solves the same system
      double acc[kSums];
#pragma unroll
      for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
      for (int c = tid; c < n; c += kOptThreads) {
        double px, py, pz, q0x, q0y, q0z;
        if constexpr (kLds) {
          px = lds[c]; py = lds[n + c]; pz = lds[2 * n + c]; q0x = lds[3 * n + c]; q0y = lds[4 * n + c]; q0z = lds[5 * n + c];
        } else {
          const size_t i = (size_t)ci[c] * 3, j = (size_t)cj[c] * 3;
          px = sp[i]; py = sp[i + 1]; pz = sp[i + 2]; q0x = tp[j]; q0y = tp[j + 1]; q0z = tp[j + 2];
        }
        const double qx = T[0] * q0x + T[1] * q0y + T[2] * q0z + T[3];
        const double qy = T[4] * q0x + T[5] * q0y + T[6] * q0z + T[7];
        const double qz = T[8] * q0x + T[9] * q0y + T[10] * q0z + T[11];
        const double rx = px - qx, ry = py - qy, rz = pz - qz;
        const double tmp = mu / (rx * rx + ry * ry + rz * rz + mu);
        const double s = tmp * tmp;
        if constexpr (kFull) {
          acc[0] += s * (qy * qy + qz * qz); acc[1] -= s * (qx * qy); acc[2] -= s * (qx * qz);
          acc[3] += s * (qx * qx + qz * qz); acc[4] -= s * (qy * qz); acc[5] += s * (qx * qx + qy * qy);
          acc[6] += s * qx; acc[7] += s * qy; acc[8] += s * qz; acc[9] += s;
          acc[10] += s * (qz * ry - qy * rz); acc[11] += s * (qx * rz - qz * rx); acc[12] += s * (qy * rx - qx * ry);
          acc[13] += s * rx; acc[14] += s * ry; acc[15] += s * rz;
        } else {
          acc[0] += s * (qx * qx + qy * qy); acc[1] += s * qx; acc[2] += s * qy; acc[3] += s;
          acc[4] += s * (qy * rx - qx * ry); acc[5] += s * rx; acc[6] += s * ry; acc[7] += s * rz;
        }
      }
#pragma unroll
      for (int k = 0; k < kSums; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
        if (lane == 0) red[it & 1][w][k] = acc[k];
      }
      __syncthreads();   // one barrier per iteration: the buffer written two iterations on is only reached through the next one
      double S[kSums];
#pragma unroll
      for (int k = 0; k < kSums; ++k) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < kOptWaves; ++q) t += red[it & 1][q][k];
        S[k] = t;
      }
      double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      bool ok;
      if constexpr (kFull) {
        // J rows [0, -qz, qy, -1, 0, 0], [qz, 0, -qx, 0, -1, 0], [-qy, qx, 0, 0, 0, -1]
        double A[6][6] = {{S[0], 0.0, 0.0, 0.0, 0.0, 0.0}, {S[1], S[3], 0.0, 0.0, 0.0, 0.0}, {S[2], S[4], S[5], 0.0, 0.0, 0.0},
                          {0.0, S[8], -S[7], S[9], 0.0, 0.0}, {-S[8], 0.0, S[6], 0.0, S[9], 0.0}, {S[7], -S[6], 0.0, 0.0, 0.0, S[9]}};
        const double b[6] = {-S[10], -S[11], -S[12], S[13], S[14], S[15]};   // -J^T r
        ok = fgr_cholesky_solve<6>(A, b, x);
      } else {
        double A[4][4] = {{S[0], 0.0, 0.0, 0.0}, {-S[2], S[3], 0.0, 0.0}, {S[1], 0.0, S[3], 0.0}, {0.0, 0.0, 0.0, S[3]}};
        const double b[4] = {-S[4], S[5], S[6], S[7]};
        double y[4];
        ok = fgr_cholesky_solve<4>(A, b, y);
        x[2] = y[0]; x[3] = y[1]; x[4] = y[2]; x[5] = y[3];
      }
      if (!ok) stopped = true;
      else {   // T <- Delta T, Delta = R_z(x2) R_y(x1) R_x(x0), t = x3..5
        double D[9];
        const double cz = cos(x[2]), sz = sin(x[2]);
        if constexpr (kFull) {
          const double cx = cos(x[0]), sx = sin(x[0]), cy = cos(x[1]), sy = sin(x[1]);
          D[0] = cz * cy; D[1] = cz * sy * sx - sz * cx; D[2] = cz * sy * cx + sz * sx;
          D[3] = sz * cy; D[4] = sz * sy * sx + cz * cx; D[5] = sz * sy * cx - cz * sx;
          D[6] = -sy; D[7] = cy * sx; D[8] = cy * cx;
        } else {
          D[0] = cz; D[1] = -sz; D[2] = 0.0; D[3] = sz; D[4] = cz; D[5] = 0.0; D[6] = 0.0; D[7] = 0.0; D[8] = 1.0;
        }
        double Tn[12];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int c = 0; c < 4; ++c) Tn[r * 4 + c] = D[r * 3] * T[c] + D[r * 3 + 1] * T[4 + c] + D[r * 3 + 2] * T[8 + c];
          Tn[r * 4 + 3] += x[3 + r];
        }
#pragma unroll
        for (int q = 0; q < 12; ++q) T[q] = Tn[q];
      }
    }
    if (f.trace && tid == 0) {
      double* tr = f.trace + ((size_t)bl * f.iterations + it) * 16;
      for (int q = 0; q < 12; ++q) tr[q] = T[q];
      tr[12] = 0.0; tr[13] = 0.0; tr[14] = 0.0; tr[15] = 1.0;
    }
    if (f.decrease_mu && (it & 3) == 0 && mu > f.max_corr_dist) mu /= f.division_factor;
  }
  if (tid == 0) {   // back to the original frame, inverted: the result maps the source onto the target
    double* out = a.out_T + (size_t)bl * 16;
    double R[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    if (ms != 0 && mt != 0) {
      const double* norm = f.norm + (size_t)bl * 8;
      const double scale = norm[6];
      double u[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) u[r] = norm[r] + scale * T[r * 4 + 3] - (T[r * 4] * norm[3] + T[r * 4 + 1] * norm[4] + T[r * 4 + 2] * norm[5]);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        R[r * 4] = T[r]; R[r * 4 + 1] = T[4 + r]; R[r * 4 + 2] = T[8 + r];
        R[r * 4 + 3] = -(T[r] * u[0] + T[4 + r] * u[1] + T[8 + r] * u[2]);
      }
    }
    for (int q = 0; q < 12; ++q) out[q] = R[q];
    out[12] = 0.0; out[13] = 0.0; out[14] = 0.0; out[15] = 1.0;
  }
}

// fitness and inlier rmse of a.out_T on the downsampled clouds against the grid of gr_grid_kernel (threshold tau), as the RANSAC validation
__global__ __launch_bounds__(kThreads) void fgr_score_kernel(const GrArgs a, const double tau)
{
  __shared__ double red[kWaves * 2];
  const int bl = blockIdx.x, tid = threadIdx.x;
  const int ms = a.m[2 * bl];
  const double* sp = a.dpts + (size_t)(2 * bl) * a.cap * 3;
  const int* gdim = a.gdim + (size_t)bl * 4;
  const int nx = gdim[0], ny = gdim[1], nz = gdim[2];
  const double mnx = a.gpar[(size_t)bl * 4], mny = a.gpar[(size_t)bl * 4 + 1], mnz = a.gpar[(size_t)bl * 4 + 2], cs = a.gpar[(size_t)bl * 4 + 3];
  const double* gx = a.gpts + (size_t)bl * a.cap * 3; const double* gy = gx + a.cap; const double* gz = gy + a.cap;
  const int* cell = a.cell + (size_t)bl * (kMaxCells + 1);
  const double tau2 = tau * tau;
  double Tl[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) Tl[q] = a.out_T[(size_t)bl * 16 + q];
  double v[2] = {0.0, 0.0};
  for (int i = tid; i < ms; i += kThreads) {
    const double sx = sp[(size_t)i * 3], sy = sp[(size_t)i * 3 + 1], sz = sp[(size_t)i * 3 + 2];
    const double qx = Tl[0] * sx + Tl[1] * sy + Tl[2] * sz + Tl[3];
    const double qy = Tl[4] * sx + Tl[5] * sy + Tl[6] * sz + Tl[7];
    const double qz = Tl[8] * sx + Tl[9] * sy + Tl[10] * sz + Tl[11];
    const double fx = floor((qx - mnx) / cs), fy = floor((qy - mny) / cs), fz = floor((qz - mnz) / cs);
    if (!(fx >= -1.0 && fx <= (double)nx && fy >= -1.0 && fy <= (double)ny && fz >= -1.0 && fz <= (double)nz)) continue;
    const int x0 = max(0, (int)fx - 1), x1 = min(nx - 1, (int)fx + 1);
    const int y0 = max(0, (int)fy - 1), y1 = min(ny - 1, (int)fy + 1);
    const int z0 = max(0, (int)fz - 1), z1 = min(nz - 1, (int)fz + 1);
    if (x0 > x1) continue;
    double best = INFINITY;
    for (int z = z0; z <= z1; ++z)
      for (int y = y0; y <= y1; ++y) {
        const int rowc = (z * ny + y) * nx;
        const int b = cell[rowc + x0], e = cell[rowc + x1 + 1];
        for (int j = b; j < e; ++j) {
          const double dx = qx - gx[j], dy = qy - gy[j], dz = qz - gz[j];
          best = fmin(best, dx * dx + dy * dy + dz * dz);
        }
      }
    if (best <= tau2) { v[0] += 1.0; v[1] += best; }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
  if ((tid & 63) == 0) { red[(tid >> 6) * 2] = v[0]; red[(tid >> 6) * 2 + 1] = v[1]; }
  __syncthreads();
  if (tid == 0) {
    double cnt = 0.0, sum = 0.0;
    for (int q = 0; q < kWaves; ++q) { cnt += red[q * 2]; sum += red[q * 2 + 1]; }
    a.out_fit[bl] = ms > 0 ? cnt / (double)ms : 0.0;
    a.out_rmse[bl] = cnt > 0.0 ? sqrt(sum / cnt) : 0.0;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

struct Carve {
  char* base; size_t at = 0;
  template <typename T> T* take(size_t count) { T* p = base ? reinterpret_cast<T*>(base + at) : nullptr; at += align_up(count * sizeof(T)); return p; }
};

// lays the stage arrays of a chunk of `pairs` pairs with clouds of at most `cap` points into `base`; returns the bytes used
size_t carve(GrArgs& a, char* base, long long pairs, long long cap, long long P2)
{
  Carve cv{base};
  const size_t C = (size_t)pairs * 2, c = (size_t)cap;
  a.cap = cap; a.P2 = P2;
  a.key = cv.take<unsigned long long>(C * P2); a.val = cv.take<int>(C * P2); a.seg = cv.take<int>(C * (c + 1));
  a.dpts = cv.take<double>(C * c * 3); a.vox = cv.take<int>(C * c * 3); a.npts = cv.take<int>(C * c); a.m = cv.take<int>(C);
  a.nrm = cv.take<double>(C * c * 3); a.nbr = cv.take<int>(C * c * kNbrStride); a.nbrc = cv.take<int>(C * c);
  a.cd2 = cv.take<double>(C * kWaves * c); a.cidx = cv.take<int>(C * kWaves * c);
  a.spfh = cv.take<double>(C * c * kBins); a.fpfh = cv.take<double>(C * c * kBins);
  a.match = cv.take<int>((size_t)pairs * c); a.cell = cv.take<int>((size_t)pairs * (kMaxCells + 1)); a.cellfill = cv.take<int>((size_t)pairs * kMaxCells);
  a.gpts = cv.take<double>((size_t)pairs * c * 3); a.gpar = cv.take<double>((size_t)pairs * 4); a.gdim = cv.take<int>((size_t)pairs * 4);
  a.err = cv.take<int>(1);
  a.out_T = cv.take<double>((size_t)pairs * 16); a.out_fit = cv.take<double>(pairs); a.out_rmse = cv.take<double>(pairs);
  a.out_iters = cv.take<long long>(pairs); a.out_vals = cv.take<int>(pairs); a.out_win = cv.take<long long>(pairs);
  return cv.at;
}

struct GrDebugOut {   // alignnet_debug_global_stages: host arrays for the stage outputs of pair 0 (stride `cap` per cloud)
  long long cap;
  int32_t* counts; double* points; int32_t* voxels; int32_t* npts; double* normals; double* spfh; double* fpfh; int32_t* matches; int64_t* win;
};

constexpr size_t kWsBudget = (size_t)3 << 29;   // 1.5 GiB of stage arrays per chunk

// stages 1-5 of a chunk of bc pairs: downsample, normals, SPFH / FPFH, the matches source -> target
void launch_front_end(alignnet_handle* h, const GrArgs& a, int bc)
{
  const int parts = bc >= 128 ? 1 : (bc >= 32 ? 4 : 16);   // workgroups per cloud of the per-point stages at small batches
  hipLaunchKernelGGL(gr_voxel_kernel, dim3(2 * bc), dim3(kThreads), 0, h->stream, a);
  hipLaunchKernelGGL(gr_neighbours_kernel<30>, dim3(2 * bc), dim3(kThreads), 0, h->stream, a, 2.0 * kVoxel, 3);
  hipLaunchKernelGGL(gr_normals_kernel, dim3(2 * bc, parts), dim3(256), 0, h->stream, a);
  hipLaunchKernelGGL(gr_neighbours_kernel<100>, dim3(2 * bc), dim3(kThreads), 0, h->stream, a, 5.0 * kVoxel, 6);
  hipLaunchKernelGGL(gr_spfh_kernel, dim3(2 * bc, parts), dim3(kThreads), 0, h->stream, a);
  hipLaunchKernelGGL(gr_fpfh_kernel, dim3(2 * bc, parts), dim3(kThreads), 0, h->stream, a);
  hipLaunchKernelGGL(gr_match_kernel<false>, dim3(bc), dim3(kThreads), 0, h->stream, a);
}

// shared driver: blobs and offsets already on the device; n1 / n2 = the cloud sizes of the B pairs (host)
int run_global(alignnet_handle* h, const std::string& name, const float* d_p0, const float* d_p1, const long long* d_off, const int* rows,
               const std::vector<long long>& n1, const std::vector<long long>& n2, int B, bool full, uint64_t seed, const int32_t* streams,
               int64_t max_iteration, int32_t max_validation, double* out_T, double* out_fit, double* out_rmse, int64_t* out_iters,
               int32_t* out_vals, const GrDebugOut* dbg)
{
  if (!out_T) return fail(h, name + ": null out_T");
  if (max_iteration < 0 || max_iteration > (1ll << 38) || max_validation < 0) return fail(h, name + ": max_iteration must be in [0, 2^38], max_validation >= 0");
  if (streams)
    for (int i = 0; i < B; ++i)
      if (streams[i] < 0 || streams[i] >= (1 << 24)) return fail(h, name + ": stream id " + std::to_string(streams[i]) + " outside [0, 2^24)");
  long long cap = 1;
  for (int i = 0; i < B; ++i) {
    if (n1[i] > 0x3fffffff || n2[i] > 0x3fffffff) return fail(h, name + ": a cloud of more than 2^30 points");
    cap = std::max(cap, std::max(n1[i], n2[i]));
  }
  long long P2 = 1;
  while (P2 < cap) P2 <<= 1;
  GrArgs a{};
  const size_t per_pair = carve(a, nullptr, 1, cap, P2);
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, kWsBudget / per_pair));
  const size_t need = carve(a, nullptr, chunk, cap, P2) + align_up((size_t)chunk * 8);
  if (grow_bytes(h, &h->globalreg_ws, &h->globalreg_ws_bytes, need)) return 1;
  const size_t used = carve(a, static_cast<char*>(h->globalreg_ws), chunk, cap, P2);
  int* d_ids = reinterpret_cast<int*>(static_cast<char*>(h->globalreg_ws) + used);   // [chunk] rows | [chunk] streams
  a.pts[0] = d_p0; a.pts[1] = d_p1; a.off = d_off;
  a.seed = seed; a.max_iteration = max_iteration; a.max_validation = max_validation;
  HIP_TRY(h, hipMemsetAsync(a.err, 0, sizeof(int), h->stream));
  static alignnet::PerDeviceOnce attr;
  if (attr.need(h->cfg.device)) {
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(gr_ransac_kernel<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(gr_ransac_kernel<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
    attr.mark(h->cfg.device);
  }
  const double tau = 1.5 * kVoxel;
  const long long lds_sure = ((long long)kLdsBytes - 4ll * (kMinLdsCells + 2)) / 24;   // targets up to this size are LDS-resident whatever they downsample to
  for (int s = 0; s < B; s += chunk) {
    const int bc = std::min(chunk, B - s);
    a.pair0 = s;
    a.rows = nullptr; a.streams = nullptr;
    if (rows) { HIP_TRY(h, hipMemcpyAsync(d_ids, rows + s, (size_t)bc * sizeof(int), hipMemcpyHostToDevice, h->stream)); a.rows = d_ids; }
    if (streams) { HIP_TRY(h, hipMemcpyAsync(d_ids + chunk, streams + s, (size_t)bc * sizeof(int), hipMemcpyHostToDevice, h->stream)); a.streams = d_ids + chunk; }
    bool hbm_path = false;
    for (int i = s; i < s + bc; ++i) hbm_path = hbm_path || n2[i] > lds_sure;
    launch_front_end(h, a, bc);
    hipLaunchKernelGGL(gr_grid_kernel, dim3(bc), dim3(kThreads), 0, h->stream, a, tau);
    if (full) {
      hipLaunchKernelGGL((gr_ransac_kernel<true, true>), dim3(bc), dim3(kThreads), kLdsBytes, h->stream, a, tau);
      if (hbm_path) hipLaunchKernelGGL((gr_ransac_kernel<true, false>), dim3(bc), dim3(kThreads), 0, h->stream, a, tau);
    } else {
      hipLaunchKernelGGL((gr_ransac_kernel<false, true>), dim3(bc), dim3(kThreads), kLdsBytes, h->stream, a, tau);
      if (hbm_path) hipLaunchKernelGGL((gr_ransac_kernel<false, false>), dim3(bc), dim3(kThreads), 0, h->stream, a, tau);
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out_T + (size_t)s * 16, a.out_T, (size_t)bc * 16 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (out_fit) HIP_TRY(h, hipMemcpyAsync(out_fit + s, a.out_fit, (size_t)bc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (out_rmse) HIP_TRY(h, hipMemcpyAsync(out_rmse + s, a.out_rmse, (size_t)bc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (out_iters) HIP_TRY(h, hipMemcpyAsync(out_iters + s, a.out_iters, (size_t)bc * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    if (out_vals) HIP_TRY(h, hipMemcpyAsync(out_vals + s, a.out_vals, (size_t)bc * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // the next chunk reuses the stage arrays
  }
  int err = 0;
  HIP_TRY(h, hipMemcpy(&err, a.err, sizeof(int), hipMemcpyDeviceToHost));
  if (err) return fail(h, name + ": a coordinate is not finite, or a cloud spans more than 2^21 voxels of 0.05 m");
  if (dbg) {   // B == 1: the stage arrays of clouds 0 (source) and 1 (target) are still in place
    const size_t c = (size_t)cap, dc = (size_t)dbg->cap;
    HIP_TRY(h, hipMemcpy(dbg->counts, a.m, 2 * sizeof(int), hipMemcpyDeviceToHost));
    for (int side = 0; side < 2; ++side) {
      const size_t m = (size_t)dbg->counts[side];
      if (m > dc) return fail(h, name + ": cap smaller than a cloud");
      if (!m) continue;
      HIP_TRY(h, hipMemcpy(dbg->points + side * dc * 3, a.dpts + side * c * 3, m * 3 * sizeof(double), hipMemcpyDeviceToHost));
      HIP_TRY(h, hipMemcpy(dbg->voxels + side * dc * 3, a.vox + side * c * 3, m * 3 * sizeof(int), hipMemcpyDeviceToHost));
      HIP_TRY(h, hipMemcpy(dbg->npts + side * dc, a.npts + side * c, m * sizeof(int), hipMemcpyDeviceToHost));
      HIP_TRY(h, hipMemcpy(dbg->normals + side * dc * 3, a.nrm + side * c * 3, m * 3 * sizeof(double), hipMemcpyDeviceToHost));
      HIP_TRY(h, hipMemcpy(dbg->spfh + side * dc * kBins, a.spfh + side * c * kBins, m * kBins * sizeof(double), hipMemcpyDeviceToHost));
      HIP_TRY(h, hipMemcpy(dbg->fpfh + side * dc * kBins, a.fpfh + side * c * kBins, m * kBins * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (dbg->counts[0]) HIP_TRY(h, hipMemcpy(dbg->matches, a.match, (size_t)dbg->counts[0] * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(dbg->win, a.out_win, sizeof(long long), hipMemcpyDeviceToHost));
  }
  return 0;
}

int gr_flags(alignnet_handle* h, const std::string& name, int32_t flags, bool* full)
{
  if (flags & ~1) return fail(h, name + ": unknown flags " + std::to_string(flags) + " (bit 0 = full rotation is the only one)");
  *full = (flags & 1) != 0;
  return 0;
}

// clouds passed from the host
int global_host(alignnet_handle* h, const char* fn, const float* points1, const float* points2, const int64_t* offsets, int32_t B, int32_t flags,
                uint64_t seed, const int32_t* streams, int64_t max_iteration, int32_t max_validation, double* out_T, double* out_fit,
                double* out_rmse, int64_t* out_iters, int32_t* out_vals, const GrDebugOut* dbg)
{
  if (!h) return 1;
  const std::string name(fn);
  bool full = false;
  if (gr_flags(h, name, flags, &full)) return 1;
  PairUpload u;
  if (upload_pairs(h, name, points1, points2, offsets, B, &u)) return 1;
  const int rc = run_global(h, name, u.pts[0].p, u.pts[1].p, u.off.p, nullptr, u.n1, u.n2, B, full, seed, streams, max_iteration,
                            max_validation, out_T, out_fit, out_rmse, out_iters, out_vals, dbg);
  hipStreamSynchronize(h->stream);   // before the uploaded clouds go
  return rc;
}

// ---- FGR host ------------------------------------------------------------------------------------------------------------------------
struct FgrParams {
  bool full, decrease_mu;
  uint64_t seed; const int32_t* streams;
  double division_factor, max_corr_dist; int32_t iterations; double tuple_scale; int32_t max_tuples;
};

struct FgrDebugOut {   // alignnet_debug_fgr_stages: host arrays for the stage outputs of pair 0 (stride `cap` per cloud)
  long long cap;
  int32_t* counts; double* points; double* fpfh; int32_t* matches; int32_t* rmatches; int32_t* cross; int32_t* tuple_source; int32_t* tuple_target;
  int64_t* tuple_trials; double* normalisation; double* trace;
};

// the FGR arrays of a chunk, behind the shared stage arrays
size_t carve_fgr(GrArgs& a, FgrArgs& f, char* base, long long pairs, long long cap, int max_tuples, int trace_iterations)
{
  Carve cv{base};
  const size_t p = (size_t)pairs, c = (size_t)cap, mtc = (size_t)max_tuples;
  a.rmatch = cv.take<int>(p * c);
  f.npts = cv.take<double>(p * 2 * c * 3); f.norm = cv.take<double>(p * 8);
  f.cross = cv.take<int>(p * c); f.counts = cv.take<int>(p * 2);
  f.ci = cv.take<int>(p * 3 * mtc + 1); f.cj = cv.take<int>(p * 3 * mtc + 1); f.ctrial = cv.take<long long>(p * mtc + 1);
  f.trials = cv.take<long long>(p);
  f.trace = trace_iterations > 0 ? cv.take<double>(p * (size_t)trace_iterations * 16) : nullptr;
  return cv.at;
}

int fgr_params(alignnet_handle* h, const std::string& name, int32_t flags, uint64_t seed, const int32_t* streams, double division_factor,
               double max_corr_dist, int32_t iterations, double tuple_scale, int32_t max_tuples, FgrParams* p)
{
  if (flags & ~(ALIGNNET_ICP_FULL_ROTATION | ALIGNNET_FGR_DECREASE_MU))
    return fail(h, name + ": unknown flags " + std::to_string(flags) + " (bit 0 = full rotation, bit 1 = decrease mu)");
  if (!(division_factor >= 1.0) || !std::isfinite(division_factor)) return fail(h, name + ": division_factor must be finite and >= 1");
  if (!(max_corr_dist > 0.0) || !std::isfinite(max_corr_dist)) return fail(h, name + ": maximum_correspondence_distance must be finite and > 0");
  if (iterations < 0 || iterations > (1 << 20)) return fail(h, name + ": iteration_number must be in [0, 2^20]");
  if (!(tuple_scale > 0.0 && tuple_scale <= 1.0)) return fail(h, name + ": tuple_scale must be in (0, 1]");
  if (max_tuples < 0 || max_tuples > (1 << 20)) return fail(h, name + ": maximum_tuple_count must be in [0, 2^20]");
  *p = FgrParams{(flags & ALIGNNET_ICP_FULL_ROTATION) != 0, (flags & ALIGNNET_FGR_DECREASE_MU) != 0, seed, streams, division_factor, max_corr_dist,
                 iterations, tuple_scale, max_tuples};
  return 0;
}

// shared driver, as run_global: blobs and offsets already on the device; n1 / n2 = the cloud sizes of the B pairs (host)
int run_fgr(alignnet_handle* h, const std::string& name, const float* d_p0, const float* d_p1, const long long* d_off, const int* rows,
            const std::vector<long long>& n1, const std::vector<long long>& n2, int B, const FgrParams& p, double* out_T, double* out_fit,
            double* out_rmse, int32_t* out_corr, int64_t* out_trials, const FgrDebugOut* dbg)
{
  if (!out_T) return fail(h, name + ": null out_T");
  if (p.streams)
    for (int i = 0; i < B; ++i)
      if (p.streams[i] < 0 || p.streams[i] >= (1 << 24)) return fail(h, name + ": stream id " + std::to_string(p.streams[i]) + " outside [0, 2^24)");
  long long cap = 1;
  for (int i = 0; i < B; ++i) {
    if (n1[i] > 0x3fffffff || n2[i] > 0x3fffffff) return fail(h, name + ": a cloud of more than 2^30 points");
    cap = std::max(cap, std::max(n1[i], n2[i]));
  }
  long long P2 = 1;
  while (P2 < cap) P2 <<= 1;
  const int trace_its = dbg ? p.iterations : 0;
  GrArgs a{}; FgrArgs f{};
  const size_t per_pair = carve(a, nullptr, 1, cap, P2) + carve_fgr(a, f, nullptr, 1, cap, p.max_tuples, trace_its);
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, kWsBudget / per_pair));
  const size_t shared_bytes = carve(a, nullptr, chunk, cap, P2);
  const size_t need = shared_bytes + carve_fgr(a, f, nullptr, chunk, cap, p.max_tuples, trace_its) + align_up((size_t)chunk * 8);
  if (grow_bytes(h, &h->globalreg_ws, &h->globalreg_ws_bytes, need)) return 1;
  char* ws = static_cast<char*>(h->globalreg_ws);
  carve(a, ws, chunk, cap, P2);
  const size_t used = shared_bytes + carve_fgr(a, f, ws + shared_bytes, chunk, cap, p.max_tuples, trace_its);
  int* d_ids = reinterpret_cast<int*>(ws + used);   // [chunk] rows | [chunk] streams
  a.pts[0] = d_p0; a.pts[1] = d_p1; a.off = d_off;
  f.seed = p.seed; f.division_factor = p.division_factor; f.max_corr_dist = p.max_corr_dist; f.tuple_scale = p.tuple_scale;
  f.iterations = p.iterations; f.max_tuples = p.max_tuples; f.decrease_mu = p.decrease_mu ? 1 : 0;
  HIP_TRY(h, hipMemsetAsync(a.err, 0, sizeof(int), h->stream));
  const bool opt_lds = 3 * (long long)p.max_tuples <= kOptLdsCorr;
  const size_t opt_lds_bytes = (size_t)3 * p.max_tuples * 48;
  static alignnet::PerDeviceOnce attr;
  if (attr.need(h->cfg.device)) {
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(fgr_optimise_kernel<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kOptLdsCorr * 48));
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(fgr_optimise_kernel<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kOptLdsCorr * 48));
    attr.mark(h->cfg.device);
  }
  std::vector<int> counts((size_t)chunk * 2);
  for (int s = 0; s < B; s += chunk) {
    const int bc = std::min(chunk, B - s);
    a.pair0 = s;
    a.rows = nullptr; a.streams = nullptr;
    if (rows) { HIP_TRY(h, hipMemcpyAsync(d_ids, rows + s, (size_t)bc * sizeof(int), hipMemcpyHostToDevice, h->stream)); a.rows = d_ids; }
    if (p.streams) { HIP_TRY(h, hipMemcpyAsync(d_ids + chunk, p.streams + s, (size_t)bc * sizeof(int), hipMemcpyHostToDevice, h->stream)); a.streams = d_ids + chunk; }
    launch_front_end(h, a, bc);
    hipLaunchKernelGGL(gr_match_kernel<true>, dim3(bc), dim3(kThreads), 0, h->stream, a);
    hipLaunchKernelGGL(fgr_tuple_kernel, dim3(bc), dim3(kThreads), 0, h->stream, a, f);
    if (opt_lds) {
      if (p.full) hipLaunchKernelGGL((fgr_optimise_kernel<true, true>), dim3(bc), dim3(kOptThreads), opt_lds_bytes, h->stream, a, f);
      else hipLaunchKernelGGL((fgr_optimise_kernel<false, true>), dim3(bc), dim3(kOptThreads), opt_lds_bytes, h->stream, a, f);
    } else {
      if (p.full) hipLaunchKernelGGL((fgr_optimise_kernel<true, false>), dim3(bc), dim3(kOptThreads), 0, h->stream, a, f);
      else hipLaunchKernelGGL((fgr_optimise_kernel<false, false>), dim3(bc), dim3(kOptThreads), 0, h->stream, a, f);
    }
    hipLaunchKernelGGL(gr_grid_kernel, dim3(bc), dim3(kThreads), 0, h->stream, a, p.max_corr_dist);
    hipLaunchKernelGGL(fgr_score_kernel, dim3(bc), dim3(kThreads), 0, h->stream, a, p.max_corr_dist);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out_T + (size_t)s * 16, a.out_T, (size_t)bc * 16 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (out_fit) HIP_TRY(h, hipMemcpyAsync(out_fit + s, a.out_fit, (size_t)bc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (out_rmse) HIP_TRY(h, hipMemcpyAsync(out_rmse + s, a.out_rmse, (size_t)bc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (out_corr) HIP_TRY(h, hipMemcpyAsync(counts.data(), f.counts, (size_t)bc * 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (out_trials) HIP_TRY(h, hipMemcpyAsync(out_trials + s, f.trials, (size_t)bc * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // the next chunk reuses the stage arrays
    if (out_corr)
      for (int i = 0; i < bc; ++i) out_corr[s + i] = 3 * counts[(size_t)i * 2 + 1];
  }
  int err = 0;
  HIP_TRY(h, hipMemcpy(&err, a.err, sizeof(int), hipMemcpyDeviceToHost));
  if (err) return fail(h, name + ": a coordinate is not finite, or a cloud spans more than 2^21 voxels of 0.05 m");
  if (dbg) {   // B == 1: the stage arrays of clouds 0 (source) and 1 (target) are still in place
    const size_t c = (size_t)cap, dc = (size_t)dbg->cap;
    HIP_TRY(h, hipMemcpy(dbg->counts, a.m, 2 * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(dbg->counts + 2, f.counts, 2 * sizeof(int), hipMemcpyDeviceToHost));
    for (int side = 0; side < 2; ++side) {
      const size_t m = (size_t)dbg->counts[side];
      if (m > dc) return fail(h, name + ": cap smaller than a cloud");
      if (!m) continue;
      HIP_TRY(h, hipMemcpy(dbg->points + side * dc * 3, a.dpts + side * c * 3, m * 3 * sizeof(double), hipMemcpyDeviceToHost));
      HIP_TRY(h, hipMemcpy(dbg->fpfh + side * dc * kBins, a.fpfh + side * c * kBins, m * kBins * sizeof(double), hipMemcpyDeviceToHost));
    }
    const size_t ms = (size_t)dbg->counts[0], mt = (size_t)dbg->counts[1], nc = (size_t)dbg->counts[2], na = (size_t)dbg->counts[3];
    if (ms && mt) {
      HIP_TRY(h, hipMemcpy(dbg->matches, a.match, ms * sizeof(int), hipMemcpyDeviceToHost));
      HIP_TRY(h, hipMemcpy(dbg->rmatches, a.rmatch, mt * sizeof(int), hipMemcpyDeviceToHost));
    }
    if (nc) HIP_TRY(h, hipMemcpy(dbg->cross, f.cross, nc * sizeof(int), hipMemcpyDeviceToHost));
    if (na) {
      HIP_TRY(h, hipMemcpy(dbg->tuple_source, f.ci, na * 3 * sizeof(int), hipMemcpyDeviceToHost));
      HIP_TRY(h, hipMemcpy(dbg->tuple_target, f.cj, na * 3 * sizeof(int), hipMemcpyDeviceToHost));
      HIP_TRY(h, hipMemcpy(dbg->tuple_trials, f.ctrial, na * sizeof(long long), hipMemcpyDeviceToHost));
    }
    HIP_TRY(h, hipMemcpy(dbg->normalisation, f.norm, 7 * sizeof(double), hipMemcpyDeviceToHost));
    if (p.iterations) HIP_TRY(h, hipMemcpy(dbg->trace, f.trace, (size_t)p.iterations * 16 * sizeof(double), hipMemcpyDeviceToHost));
  }
  return 0;
}

// clouds passed from the host
int fgr_host(alignnet_handle* h, const std::string& name, const float* points1, const float* points2, const int64_t* offsets, int32_t B,
             const FgrParams& p, double* out_T, double* out_fit, double* out_rmse, int32_t* out_corr, int64_t* out_trials, const FgrDebugOut* dbg)
{
  PairUpload u;
  if (upload_pairs(h, name, points1, points2, offsets, B, &u)) return 1;
  const int rc = run_fgr(h, name, u.pts[0].p, u.pts[1].p, u.off.p, nullptr, u.n1, u.n2, B, p, out_T, out_fit, out_rmse, out_corr, out_trials, dbg);
  hipStreamSynchronize(h->stream);   // before the uploaded clouds go
  return rc;
}

}  // namespace

extern "C" void alignnet_globalreg_free(alignnet_handle* h)
{
  if (!h || !h->globalreg_ws) return;
  hipFree(h->globalreg_ws);
  h->globalreg_ws = nullptr; h->globalreg_ws_bytes = 0;
}

extern "C" int alignnet_global_register(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets, int32_t B,
                                        int32_t flags, uint64_t seed, const int32_t* streams, int64_t max_iteration, int32_t max_validation,
                                        double* out_T, double* out_fitness, double* out_rmse, int64_t* out_iterations, int32_t* out_validations)
{
  return global_host(h, "alignnet_global_register", points1, points2, offsets, B, flags, seed, streams, max_iteration, max_validation, out_T,
                     out_fitness, out_rmse, out_iterations, out_validations, nullptr);
}

extern "C" int alignnet_global_register_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, int32_t flags, uint64_t seed,
                                                const int32_t* streams, int64_t max_iteration, int32_t max_validation, double* out_T,
                                                double* out_fitness, double* out_rmse, int64_t* out_iterations, int32_t* out_validations)
{
  if (!h) return 1;
  const std::string name("alignnet_global_register_dataset");
  bool full = false;
  if (gr_flags(h, name, flags, &full)) return 1;
  alignnet::DatasetTables t;
  if (!alignnet_dataset_tables(h, &t)) return fail(h, name + ": no dataset uploaded");
  if (!rows || B < 1) return fail(h, name + ": null rows or B < 1");
  for (int i = 0; i < B; ++i)
    if (rows[i] < 0 || rows[i] >= t.n) return fail(h, name + ": row " + std::to_string(rows[i]) + " out of range");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  std::vector<long long> off((size_t)(t.n + 1) * 2), n1(B), n2(B);   // the cloud sizes size the stage arrays
  HIP_TRY(h, hipMemcpy(off.data(), t.off, off.size() * sizeof(long long), hipMemcpyDeviceToHost));
  for (int i = 0; i < B; ++i) {
    n1[i] = off[((size_t)rows[i] + 1) * 2] - off[(size_t)rows[i] * 2];
    n2[i] = off[((size_t)rows[i] + 1) * 2 + 1] - off[(size_t)rows[i] * 2 + 1];
  }
  return run_global(h, name, t.pts[0], t.pts[1], t.off, rows, n1, n2, B, full, seed, streams, max_iteration, max_validation, out_T, out_fitness,
                    out_rmse, out_iterations, out_validations, nullptr);
}

extern "C" int alignnet_debug_global_stages(alignnet_handle* h, const float* points1, int64_t n1, const float* points2, int64_t n2, int32_t flags,
                                            uint64_t seed, int32_t stream, int64_t max_iteration, int32_t max_validation, int64_t cap,
                                            int32_t* counts, double* points, int32_t* voxels, int32_t* voxel_points, double* normals, double* spfh,
                                            double* fpfh, int32_t* matches, int64_t* winning_iteration, double* out_T, double* out_fitness,
                                            double* out_rmse, int64_t* out_iterations, int32_t* out_validations)
{
  if (!h) return 1;
  if (n1 < 0 || n2 < 0 || cap < n1 || cap < n2) return fail(h, "alignnet_debug_global_stages: cap must hold both clouds");
  if (!counts || !points || !voxels || !voxel_points || !normals || !spfh || !fpfh || !matches || !winning_iteration)
    return fail(h, "alignnet_debug_global_stages: null output");
  const int64_t offsets[4] = {0, 0, n1, n2};
  const GrDebugOut dbg{cap, counts, points, voxels, voxel_points, normals, spfh, fpfh, matches, winning_iteration};
  return global_host(h, "alignnet_debug_global_stages", points1, points2, offsets, 1, flags, seed, &stream, max_iteration, max_validation, out_T,
                     out_fitness, out_rmse, out_iterations, out_validations, &dbg);
}

extern "C" int alignnet_fgr_register(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets, int32_t B, int32_t flags,
                                     uint64_t seed, const int32_t* streams, double division_factor, double maximum_correspondence_distance,
                                     int32_t iteration_number, double tuple_scale, int32_t maximum_tuple_count, double* out_T, double* out_fitness,
                                     double* out_rmse, int32_t* out_correspondences, int64_t* out_trials)
{
  if (!h) return 1;
  const std::string name("alignnet_fgr_register");
  FgrParams p;
  if (fgr_params(h, name, flags, seed, streams, division_factor, maximum_correspondence_distance, iteration_number, tuple_scale, maximum_tuple_count, &p))
    return 1;
  return fgr_host(h, name, points1, points2, offsets, B, p, out_T, out_fitness, out_rmse, out_correspondences, out_trials, nullptr);
}

extern "C" int alignnet_fgr_register_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, int32_t flags, uint64_t seed, const int32_t* streams,
                                             double division_factor, double maximum_correspondence_distance, int32_t iteration_number,
                                             double tuple_scale, int32_t maximum_tuple_count, double* out_T, double* out_fitness, double* out_rmse,
                                             int32_t* out_correspondences, int64_t* out_trials)
{
  if (!h) return 1;
  const std::string name("alignnet_fgr_register_dataset");
  FgrParams p;
  if (fgr_params(h, name, flags, seed, streams, division_factor, maximum_correspondence_distance, iteration_number, tuple_scale, maximum_tuple_count, &p))
    return 1;
  alignnet::DatasetTables t;
  if (!alignnet_dataset_tables(h, &t)) return fail(h, name + ": no dataset uploaded");
  if (!rows || B < 1) return fail(h, name + ": null rows or B < 1");
  for (int i = 0; i < B; ++i)
    if (rows[i] < 0 || rows[i] >= t.n) return fail(h, name + ": row " + std::to_string(rows[i]) + " out of range");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  std::vector<long long> off((size_t)(t.n + 1) * 2), n1(B), n2(B);   // the cloud sizes size the stage arrays
  HIP_TRY(h, hipMemcpy(off.data(), t.off, off.size() * sizeof(long long), hipMemcpyDeviceToHost));
  for (int i = 0; i < B; ++i) {
    n1[i] = off[((size_t)rows[i] + 1) * 2] - off[(size_t)rows[i] * 2];
    n2[i] = off[((size_t)rows[i] + 1) * 2 + 1] - off[(size_t)rows[i] * 2 + 1];
  }
  return run_fgr(h, name, t.pts[0], t.pts[1], t.off, rows, n1, n2, B, p, out_T, out_fitness, out_rmse, out_correspondences, out_trials, nullptr);
}

extern "C" int alignnet_debug_fgr_stages(alignnet_handle* h, const float* points1, int64_t n1, const float* points2, int64_t n2, int32_t flags,
                                         uint64_t seed, int32_t stream, double division_factor, double maximum_correspondence_distance,
                                         int32_t iteration_number, double tuple_scale, int32_t maximum_tuple_count, int64_t cap, int32_t* counts,
                                         double* points, double* fpfh, int32_t* matches, int32_t* reverse_matches, int32_t* cross,
                                         int32_t* tuple_source, int32_t* tuple_target, int64_t* tuple_trials, double* normalisation, double* trace,
                                         double* out_T, double* out_fitness, double* out_rmse, int32_t* out_correspondences, int64_t* out_trials)
{
  if (!h) return 1;
  const std::string name("alignnet_debug_fgr_stages");
  if (n1 < 0 || n2 < 0 || cap < n1 || cap < n2) return fail(h, name + ": cap must hold both clouds");
  if (!counts || !points || !fpfh || !matches || !reverse_matches || !cross || !tuple_source || !tuple_target || !tuple_trials || !normalisation || !trace)
    return fail(h, name + ": null output");
  FgrParams p;
  if (fgr_params(h, name, flags, seed, &stream, division_factor, maximum_correspondence_distance, iteration_number, tuple_scale, maximum_tuple_count, &p))
    return 1;
  const int64_t offsets[4] = {0, 0, n1, n2};
  const FgrDebugOut dbg{cap, counts, points, fpfh, matches, reverse_matches, cross, tuple_source, tuple_target, tuple_trials, normalisation, trace};
  return fgr_host(h, name, points1, points2, offsets, 1, p, out_T, out_fitness, out_rmse, out_correspondences, out_trials, &dbg);
}
