// Go-ICP style global registration of a pair of clouds (the reference's `goicp` variant, icp.py:146-147: named and left `assert False`), gfx950 only:
// a level-synchronous branch-and-bound over yaw and a translation box (rotation about z only: four degrees of freedom) on subsampled working
// sets, with a lower bound on what any pose of the box can reach.  The answer does not depend on a start, and it comes with a certificate
// (error - lower_bound).  The computation is DEFINED by tests/goicp_ref.py, whose header states the problem, the bounds and the search; this
// file follows it decision by decision.  Every decision and every sum is fp64 on coordinates centred in fp64.
//
// Kernels, over a chunk of pairs whose buffers fit kGoBudget, all arrays in a workspace owned by the handle:
//   goicp_prep_kernel    one workgroup per cloud: the working set, its mean (fixed-order sums), the centred points with rho (source) or |q|^2
//                        (target), and the float32 working sets that the ICP starts run on
//   goicp_eval_kernel    THE HOT PATH.  A workgroup (four waves) stages the pair's centred target in LDS once, [x y z |q|^2] in fp64, and
//                        takes a share of the pair's frontier, one node per wave at a time.  Per 16 source points x 16 targets one
//                        v_mfma_f64_16x16x4_f64 gives |q|^2 - 2 x.q (A row = [-2x -2y -2z 1], B column = [qx qy qz |q|^2]: K = 3 padded to
//                        4 carries the norm); the running minimum keeps the target's index, and the distance that enters the sums is then
//                        taken by differences from that target (the expansion only selects: its cancellation never reaches a result).
//                        ub and lb of a node are summed by one wave in a fixed order, so a node's numbers depend on nothing but the node.
//   goicp_best_kernel    one workgroup per pair: the lowest ub of the level, lowest frontier index on a tie (two-pass: lanes, then a tree)
//   goicp_expand_kernel  one workgroup per pair: counts the survivors (lb < best - eps), decides the stop status, and otherwise writes
//                        the children of the survivors, in their parents' order, by a block scan
// The level loop is on the host: at most max_levels <= 24 rounds, one read-back of the chunk's frontier sizes per round, which sizes the
// next evaluation's grid.  No kernel waits on another workgroup; every device loop is bounded by an argument or by a capacity the host
// checked; nothing is allocated inside the loop.
#include "engine.h"
#include "host_util.h"
#include <cmath>
#include <limits>
#include <vector>

namespace {

constexpr int kGoThreads = 256, kGoWaves = kGoThreads / 64;
constexpr int kGoStage = 2048;                      // targets staged in LDS at once: 64 KiB, two workgroups per CU
constexpr int kGoExpThreads = 1024;
constexpr int kGoLevels = ALIGNNET_GOICP_MAX_LEVELS;
constexpr size_t kGoBudget = (size_t)1 << 30;       // bytes of frontier and stage buffers per chunk of pairs
constexpr int kGoTargetWgs = 2048;                  // workgroups an evaluation aims at (256 CUs x 2 resident x 4 deep)
constexpr double kGoPi = 3.14159265358979323846;
constexpr double kGoFar = 1e300;                    // |q|^2 of the padding columns: never the minimum

typedef double go_f64x4 __attribute__((ext_vector_type(4)));

struct GoLevel {        // what all nodes of a level share
  int depth[4];         // halvings of (theta, x, y, z)
  int split[4];         // 1: the dimension is halved after this level
  double w[4];          // half-widths of a node
  double gs, an;        // gamma_i = gs rho_i + an
  int level, nchild;
};

struct GoArgs {
  const float* pts[2]; const long long* off; const int* rows;   // the call's clouds
  int pair0, ms, mt, cap, stage, starts;
  alignnet_goicp_params prm;
  long long* wsoff;     // [P + 1][2] row offsets of the float32 working sets
  float* ws[2];         // the float32 working sets, concatenated
  double* sc;           // [P][ms][4] centred source x y z rho
  double* qc;           // [P][mt][4] centred target x y z |q|^2
  double* mean;         // [P][2][3]
  int *ns, *nq;         // [P] working-set sizes
  int* nodes[2];        // [P][cap][4] frontier, ping-pong
  double *ub, *lb;      // [P][cap]
  int* count;           // [P] frontier size (0: the pair has stopped)
  double *best, *pose, *lower;   // [P], [P][4], [P]
  int* status;          // [P]
  int *evaluated, *survived;     // [P][kGoLevels]
  double* out_T;        // [P][16]
  double *fitness, *f_ub, *f_lb; int* one;   // [P] each: the share of S within fitness_radius at the returned pose (one: 1 unless empty)
  // the ICP starts
  double *s_init, *s_out, *s_fit, *s_rmse, *s_pose, *s_ub, *s_lb;   // [P starts] x 16, 16, 1, 1, 4, 1, 1
  int *s_iters, *s_rows, *s_valid, *s_count; long long* s_wsoff;      // [P starts], .., .., [P], [2 P starts]
};

__device__ __forceinline__ double go_centre(int c, int depth, double w) { return (double)(2 * c + 1 - (1 << depth)) * w; }

// ---- preparation ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void goicp_prep_kernel(const GoArgs a)
{
  __shared__ double red[3][256];
  const int p = blockIdx.x, side = blockIdx.y, tid = threadIdx.x;
  const int row = a.rows ? a.rows[a.pair0 + p] : a.pair0 + p;
  const long long o = a.off[(size_t)row * 2 + side], n = a.off[(size_t)(row + 1) * 2 + side] - o;
  const int cap = side ? a.mt : a.ms;
  const int m = (int)(n < cap ? n : cap);
  const float* src = a.pts[side] + (size_t)o * 3;
  float* dst = a.ws[side] + (size_t)a.wsoff[(size_t)p * 2 + side] * 3;
  auto pick = [&](int i) -> long long { return n <= cap ? (long long)i : ((long long)i * n) / cap; };
  double f[3] = {0.0, 0.0, 0.0}, s[3] = {0.0, 0.0, 0.0};
  if (m > 0)
    for (int k = 0; k < 3; ++k) f[k] = (double)src[pick(0) * 3 + k];
  for (int i = tid; i < m; i += 256) {
    const long long j = pick(i);
    for (int k = 0; k < 3; ++k) {
      const float v = src[j * 3 + k];
      dst[(size_t)i * 3 + k] = v;
      s[k] += (double)v - f[k];
    }
  }
  for (int k = 0; k < 3; ++k) red[k][tid] = s[k];
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h)
      for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + h];
    __syncthreads();
  }
  double c[3];
  for (int k = 0; k < 3; ++k) c[k] = m > 0 ? f[k] + red[k][0] / (double)m : 0.0;
  if (tid == 0) {
    for (int k = 0; k < 3; ++k) a.mean[((size_t)p * 2 + side) * 3 + k] = c[k];
    (side ? a.nq : a.ns)[p] = m;
  }
  double* out = side ? a.qc + (size_t)p * a.mt * 4 : a.sc + (size_t)p * a.ms * 4;
  for (int i = tid; i < m; i += 256) {
    const long long j = pick(i);
    const double x = (double)src[j * 3] - c[0], y = (double)src[j * 3 + 1] - c[1], z = (double)src[j * 3 + 2] - c[2];
    out[(size_t)i * 4] = x; out[(size_t)i * 4 + 1] = y; out[(size_t)i * 4 + 2] = z;
    out[(size_t)i * 4 + 3] = side ? x * x + y * y + z * z : sqrt(x * x + y * y);
  }
}

// per pair: the root frontier or EMPTY, and the inits of the ICP starts (rotation 2 pi k / starts about c1, then t0)
__global__ void goicp_init_kernel(const GoArgs a, const int P)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const bool empty = a.ns[p] == 0 || a.nq[p] == 0;
  a.count[p] = empty ? 0 : 1;
  a.status[p] = empty ? ALIGNNET_GOICP_EMPTY : -1;
  a.best[p] = empty ? 0.0 : std::numeric_limits<double>::infinity();
  a.lower[p] = 0.0;
  a.fitness[p] = 0.0; a.one[p] = empty ? 0 : 1;
  for (int k = 0; k < 4; ++k) { a.pose[(size_t)p * 4 + k] = 0.0; a.nodes[0][(size_t)p * a.cap * 4 + k] = 0; }
  for (int l = 0; l < kGoLevels; ++l) { a.evaluated[(size_t)p * kGoLevels + l] = 0; a.survived[(size_t)p * kGoLevels + l] = 0; }
  if (a.starts > 0) a.s_count[p] = empty ? 0 : a.starts;
  const double* c1 = a.mean + (size_t)p * 6;
  const double* cq = c1 + 3;
  for (int k = 0; k < a.starts; ++k) {
    const double ang = 2.0 * kGoPi * (double)k / (double)a.starts, c = cos(ang), s = sin(ang);
    double* T = a.s_init + ((size_t)p * a.starts + k) * 16;
    for (int e = 0; e < 16; ++e) T[e] = (e % 5 == 0) ? 1.0 : 0.0;
    T[0] = c; T[1] = -s; T[4] = s; T[5] = c;
    T[3] = cq[0] - (c * c1[0] - s * c1[1]); T[7] = cq[1] - (s * c1[0] + c * c1[1]); T[11] = cq[2] - c1[2];
    a.s_rows[(size_t)p * a.starts + k] = p;
  }
}

// the transforms the ICP starts ended at, as poses of this parametrisation; valid when inside the domain
__global__ void goicp_start_pose_kernel(const GoArgs a, const int n)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  const int p = b / a.starts;
  const double* T = a.s_out + (size_t)b * 16;
  const double* c1 = a.mean + (size_t)p * 6;
  const double* cq = c1 + 3;
  double q[4];
  q[0] = atan2(T[4], T[0]);
  for (int k = 0; k < 3; ++k) q[1 + k] = T[k * 4] * c1[0] + T[k * 4 + 1] * c1[1] + T[k * 4 + 2] * c1[2] + T[k * 4 + 3] - cq[k];
  bool ok = fabs(q[0]) <= a.prm.yaw_half;
  for (int k = 0; k < 3; ++k) ok = ok && fabs(q[1 + k]) <= a.prm.t_half[k];
  for (int k = 0; k < 4; ++k) a.s_pose[(size_t)b * 4 + k] = ok ? q[k] : 0.0;
  a.s_valid[b] = ok ? 1 : 0;
}

// the exact E of the valid starts competes for the best pose: in start order, strictly smaller replaces
__global__ void goicp_start_best_kernel(const GoArgs a, const int P)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P || a.s_count[p] == 0) return;
  for (int k = 0; k < a.starts; ++k) {
    const size_t b = (size_t)p * a.starts + k;
    if (a.s_valid[b] && a.s_ub[b] < a.best[p]) {
      a.best[p] = a.s_ub[b];
      for (int e = 0; e < 4; ++e) a.pose[(size_t)p * 4 + e] = a.s_pose[b * 4 + e];
    }
  }
}

// ---- node evaluation -----------------------------------------------------------------------------------------------------------------
struct GoEval {
  const double* sc; const double* qc; const int* ns; const int* nq;
  const int* nodes; const double* poses;   // the nodes as integer coordinates, or (poses != null) as explicit (theta, t)
  const int* count; double* ub; double* lb;
  double* fit; double fit_radius;           // fit != null: the share of the source within fit_radius of its nearest target
  int ms, mt, cap, stage, npw, rounds;      // cap: row stride of nodes / poses / ub / lb; npw = rounds * kGoWaves nodes per workgroup
  double trunc;
  GoLevel lv;
};

__global__ __launch_bounds__(kGoThreads) void goicp_eval_kernel(const GoEval a)
{
  extern __shared__ double go_lq[];   // [stage][4]
  const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, kq = lane >> 4;
  const int cnt = min(a.count[p], a.cap), base = blockIdx.x * a.npw;
  if (base >= cnt) return;   // (the whole workgroup)
  const int ns = min(a.ns[p], a.ms), nq = min(a.nq[p], a.mt);
  const double* S = a.sc + (size_t)p * a.ms * 4;
  const double* Q = a.qc + (size_t)p * a.mt * 4;
  const int nchunks = (nq + a.stage - 1) / a.stage, stiles = (ns + 15) >> 4;
  const double inf = std::numeric_limits<double>::infinity();
  auto stage = [&](int c) -> int {   // chunk c of the target into LDS, padded to whole tiles; returns its tiles
    const int q0 = c * a.stage, n = min(a.stage, nq - q0), tiles = (n + 15) >> 4;
    for (int e = tid; e < tiles * 64; e += kGoThreads) {
      const int j = e >> 2, k = e & 3;
      go_lq[e] = j < n ? Q[(size_t)(q0 + j) * 4 + k] : (k == 3 ? kGoFar : 0.0);
    }
    return tiles;
  };
  int tiles0 = 0;
  if (nchunks == 1) { tiles0 = stage(0); __syncthreads(); }
  for (int r = 0; r < a.rounds; ++r) {
    const int n = base + r * kGoWaves + wave;
    const bool live = n < cnt;   // (per wave; a wave without a node walks the same loops for the barriers' sake)
    double th = 0.0, tx = 0.0, ty = 0.0, tz = 0.0;
    if (live) {
      if (a.poses) {
        const double* q = a.poses + ((size_t)p * a.cap + n) * 4;
        th = q[0]; tx = q[1]; ty = q[2]; tz = q[3];
      } else {
        const int* c = a.nodes + ((size_t)p * a.cap + n) * 4;
        th = go_centre(c[0], a.lv.depth[0], a.lv.w[0]); tx = go_centre(c[1], a.lv.depth[1], a.lv.w[1]);
        ty = go_centre(c[2], a.lv.depth[2], a.lv.w[2]); tz = go_centre(c[3], a.lv.depth[3], a.lv.w[3]);
      }
    }
    const double sn = sin(th), cs = cos(th);
    double ubacc = 0.0, lbacc = 0.0, fitacc = 0.0;
    for (int st = 0; st < stiles; ++st) {
      const int i = st * 16 + col;   // the source point of this lane's A row
      double x = 0.0, y = 0.0, z = 0.0, rho = 0.0;
      if (i < ns) {
        const double sx = S[(size_t)i * 4], sy = S[(size_t)i * 4 + 1];
        x = cs * sx - sn * sy + tx; y = sn * sx + cs * sy + ty; z = S[(size_t)i * 4 + 2] + tz; rho = S[(size_t)i * 4 + 3];
      }
      const double aop = kq == 0 ? -2.0 * x : (kq == 1 ? -2.0 * y : (kq == 2 ? -2.0 * z : 1.0));
      double bd2[4] = {inf, inf, inf, inf};   // D rows kq + 4 r of the tile: the exact squared distance to the nearest target so far
      for (int c = 0; c < nchunks; ++c) {
        int tiles = tiles0;
        if (nchunks > 1) { __syncthreads(); tiles = stage(c); __syncthreads(); }
        double bv[4] = {inf, inf, inf, inf};
        int bj[4] = {0, 0, 0, 0};
        for (int jt = 0; jt < tiles; ++jt) {
          const double b = go_lq[(jt * 16 + col) * 4 + kq];
          const go_f64x4 zero = {0.0, 0.0, 0.0, 0.0};
          const go_f64x4 acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aop, b, zero, 0, 0, 0);
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (acc[q] < bv[q]) { bv[q] = acc[q]; bj[q] = jt; }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          double v = bv[q];
          int j = bj[q] * 16 + col;
#pragma unroll
          for (int m = 1; m < 16; m <<= 1) {   // over the 16 columns held by the lanes of this kq
            const double ov = __shfl_xor(v, m);
            const int oj = __shfl_xor(j, m);
            if (ov < v || (ov == v && oj < j)) { v = ov; j = oj; }
          }
          const int srcl = kq + 4 * q;   // a lane that holds this row's point
          const double xr = __shfl(x, srcl), yr = __shfl(y, srcl), zr = __shfl(z, srcl);
          if (tiles > 0) {
            const double dx = xr - go_lq[j * 4], dy = yr - go_lq[j * 4 + 1], dz = zr - go_lq[j * 4 + 2];
            bd2[q] = fmin(bd2[q], dx * dx + dy * dy + dz * dz);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double rr = __shfl(rho, kq + 4 * q);
        if (st * 16 + kq + 4 * q < ns) {
          const double d = sqrt(bd2[q]);
          const double u = fmin(d, a.trunc), l = fmin(fmax(d - (a.lv.gs * rr + a.lv.an), 0.0), a.trunc);
          ubacc += u * u; lbacc += l * l;
          fitacc += d <= a.fit_radius ? 1.0 : 0.0;
        }
      }
    }
    // the four row groups of the wave (every lane of a group holds the group's sum)
    ubacc += __shfl_xor(ubacc, 16); ubacc += __shfl_xor(ubacc, 32);
    lbacc += __shfl_xor(lbacc, 16); lbacc += __shfl_xor(lbacc, 32);
    fitacc += __shfl_xor(fitacc, 16); fitacc += __shfl_xor(fitacc, 32);
    if (live && lane == 0) {
      a.ub[(size_t)p * a.cap + n] = ubacc; a.lb[(size_t)p * a.cap + n] = lbacc;
      if (a.fit) a.fit[(size_t)p * a.cap + n] = fitacc / (double)ns;
    }
  }
}

// ---- best pose of a level ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void goicp_best_kernel(const GoArgs a, const GoLevel lv, const int src)
{
  __shared__ double rv[256];
  __shared__ int ri[256];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int cnt = min(a.count[p], a.cap);
  if (cnt == 0) return;
  const double* ub = a.ub + (size_t)p * a.cap;
  double v = std::numeric_limits<double>::infinity();
  int idx = 0x7fffffff;
  for (int i = tid; i < cnt; i += 256)
    if (ub[i] < v) { v = ub[i]; idx = i; }
  rv[tid] = v; ri[tid] = idx;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h && (rv[tid + h] < rv[tid] || (rv[tid + h] == rv[tid] && ri[tid + h] < ri[tid]))) { rv[tid] = rv[tid + h]; ri[tid] = ri[tid + h]; }
    __syncthreads();
  }
  if (tid == 0) {
    a.evaluated[(size_t)p * kGoLevels + lv.level] = cnt;
    if (ri[0] < cnt && rv[0] < a.best[p]) {
      a.best[p] = rv[0];
      const int* c = a.nodes[src] + ((size_t)p * a.cap + ri[0]) * 4;
      for (int k = 0; k < 4; ++k) a.pose[(size_t)p * 4 + k] = go_centre(c[k], lv.depth[k], lv.w[k]);
    }
  }
}

// ---- prune, compact, expand ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGoExpThreads) void goicp_expand_kernel(const GoArgs a, const GoLevel lv, const int src)
{
  __shared__ double rmin[kGoExpThreads];
  __shared__ int rcnt[kGoExpThreads];
  __shared__ int wsum[kGoExpThreads / 64];
  __shared__ int go;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cnt = min(a.count[p], a.cap);
  if (cnt == 0) return;
  const double* lb = a.lb + (size_t)p * a.cap;
  const double thr = a.best[p] - a.prm.mse_thresh * (double)a.ns[p];
  // pass 1: the survivors and their lowest bound
  double mn = std::numeric_limits<double>::infinity();
  int m = 0;
  for (int i = tid; i < cnt; i += kGoExpThreads)
    if (lb[i] < thr) { ++m; mn = fmin(mn, lb[i]); }
  rmin[tid] = mn; rcnt[tid] = m;
  __syncthreads();
  for (int h = kGoExpThreads / 2; h > 0; h >>= 1) {
    if (tid < h) { rmin[tid] = fmin(rmin[tid], rmin[tid + h]); rcnt[tid] += rcnt[tid + h]; }
    __syncthreads();
  }
  if (tid == 0) {
    const int surv = rcnt[0];
    a.survived[(size_t)p * kGoLevels + lv.level] = surv;
    int st = -1;
    if (surv == 0) st = ALIGNNET_GOICP_CERTIFIED;
    else if (lv.nchild == 1) st = ALIGNNET_GOICP_RESOLUTION;
    else if (lv.level + 1 >= a.prm.max_levels) st = ALIGNNET_GOICP_LEVELS;
    else if ((long long)surv * lv.nchild > (long long)a.prm.max_frontier) st = ALIGNNET_GOICP_OVERFLOW;
    if (st >= 0) {
      a.status[p] = st;
      a.lower[p] = fmin(thr, rmin[0]);   // (no survivor: rmin is +inf)
      a.count[p] = 0;
    } else {
      a.count[p] = surv * lv.nchild;
    }
    go = st < 0;
  }
  __syncthreads();
  if (!go) return;
  // pass 2: the children of the survivors, in their parents' order (max_frontier <= cap: the host checked)
  const int* in = a.nodes[src] + (size_t)p * a.cap * 4;
  int* out = a.nodes[src ^ 1] + (size_t)p * a.cap * 4;
  int running = 0;
  for (int b0 = 0; b0 < cnt; b0 += kGoExpThreads) {
    const int i = b0 + tid;
    const bool keep = i < cnt && lb[i] < thr;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int before = running, total = 0;
    for (int w = 0; w < kGoExpThreads / 64; ++w) { if (w < wave) before += wsum[w]; total += wsum[w]; }
    if (keep) {
      const int rank = before + __popcll(bal & ((1ull << lane) - 1ull));
      const int c0 = in[(size_t)i * 4], c1 = in[(size_t)i * 4 + 1], c2 = in[(size_t)i * 4 + 2], c3 = in[(size_t)i * 4 + 3];
      for (int ch = 0; ch < lv.nchild; ++ch) {
        int bits = ch, c[4] = {c0, c1, c2, c3};
        for (int k = 3; k >= 0; --k)
          if (lv.split[k]) { c[k] = 2 * c[k] + (bits & 1); bits >>= 1; }
        int* o = out + ((size_t)rank * lv.nchild + ch) * 4;
        o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = c[3];
      }
    }
    running += total;
    __syncthreads();
  }
}

// the result of every pair: x -> Rz(theta)(x - c1) + cq + t as a 4x4 about the origin
__global__ void goicp_finish_kernel(const GoArgs a, const int P)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  double* T = a.out_T + (size_t)p * 16;
  for (int e = 0; e < 16; ++e) T[e] = (e % 5 == 0) ? 1.0 : 0.0;
  if (a.status[p] == ALIGNNET_GOICP_EMPTY) return;
  const double* q = a.pose + (size_t)p * 4;
  const double* c1 = a.mean + (size_t)p * 6;
  const double* cq = c1 + 3;
  const double c = cos(q[0]), s = sin(q[0]);
  T[0] = c; T[1] = -s; T[4] = s; T[5] = c;
  T[3] = cq[0] + q[1] - (c * c1[0] - s * c1[1]); T[7] = cq[1] + q[2] - (s * c1[0] + c * c1[1]); T[11] = cq[2] + q[3] - c1[2];
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
size_t go_up(size_t x) { return (x + 255) & ~(size_t)255; }

struct GoCarve {
  char* base; size_t at = 0;
  template <typename T> T* take(size_t count) { T* p = base ? reinterpret_cast<T*>(base + at) : nullptr; at += go_up(count * sizeof(T)); return p; }
};

// lays the arrays of a chunk of P pairs into `base` (null: sizes only); returns the bytes used
size_t go_carve(GoArgs& a, char* base, size_t P)
{
  GoCarve cv{base};
  const size_t ms = (size_t)a.ms, mt = (size_t)a.mt, cap = (size_t)a.cap, st = (size_t)a.starts;
  a.wsoff = cv.take<long long>((P + 1) * 2);
  a.ws[0] = cv.take<float>(P * ms * 3); a.ws[1] = cv.take<float>(P * mt * 3);
  a.sc = cv.take<double>(P * ms * 4); a.qc = cv.take<double>(P * mt * 4); a.mean = cv.take<double>(P * 6);
  a.ns = cv.take<int>(P); a.nq = cv.take<int>(P);
  a.nodes[0] = cv.take<int>(P * cap * 4); a.nodes[1] = cv.take<int>(P * cap * 4);
  a.ub = cv.take<double>(P * cap); a.lb = cv.take<double>(P * cap);
  a.count = cv.take<int>(P); a.best = cv.take<double>(P); a.pose = cv.take<double>(P * 4); a.lower = cv.take<double>(P);
  a.status = cv.take<int>(P); a.evaluated = cv.take<int>(P * kGoLevels); a.survived = cv.take<int>(P * kGoLevels);
  a.out_T = cv.take<double>(P * 16);
  a.fitness = cv.take<double>(P); a.f_ub = cv.take<double>(P); a.f_lb = cv.take<double>(P); a.one = cv.take<int>(P);
  a.s_init = cv.take<double>(P * st * 16); a.s_out = cv.take<double>(P * st * 16); a.s_fit = cv.take<double>(P * st); a.s_rmse = cv.take<double>(P * st);
  a.s_pose = cv.take<double>(P * st * 4); a.s_ub = cv.take<double>(P * st); a.s_lb = cv.take<double>(P * st);
  a.s_iters = cv.take<int>(P * st); a.s_rows = cv.take<int>(P * st); a.s_valid = cv.take<int>(P * st); a.s_count = cv.take<int>(P);
  a.s_wsoff = cv.take<long long>(2 * P * st);
  return cv.at;
}

int go_check_params(alignnet_handle* h, const std::string& name, const alignnet_goicp_params* q)
{
  if (!q) return fail(h, name + ": null params");
  if (q->flags != 0) return fail(h, name + ": flags must be 0 (the search is z-constrained: yaw and translation only)");
  bool ok = q->yaw_half >= 0.0 && q->yaw_half <= kGoPi && q->yaw_res > 0.0 && q->t_res > 0.0 && q->trunc > 0.0 && q->mse_thresh >= 0.0 &&
            std::isfinite(q->mse_thresh) && std::isfinite(q->yaw_res) && std::isfinite(q->t_res);
  for (int k = 0; k < 3; ++k) ok = ok && q->t_half[k] >= 0.0 && std::isfinite(q->t_half[k]);
  if (!ok) return fail(h, name + ": yaw_half in [0, pi], t_half >= 0, yaw_res > 0, t_res > 0, trunc > 0 (may be inf), mse_thresh >= 0");
  if (q->max_source < 1 || q->max_source > (1 << 16) || q->max_target < 1 || q->max_target > (1 << 20))
    return fail(h, name + ": max_source in [1, 2^16], max_target in [1, 2^20]");
  if (q->max_frontier < 1 || q->max_frontier > (1 << 24) || q->max_levels < 1 || q->max_levels > kGoLevels)
    return fail(h, name + ": max_frontier in [1, 2^24], max_levels in [1, " + std::to_string(kGoLevels) + "]");
  if (q->starts < 0 || q->starts > 64 || q->start_its < 0 || (q->starts > 0 && !(q->start_radius > 0.0)))
    return fail(h, name + ": starts in [0, 64], start_its >= 0, start_radius > 0");
  if (!(q->fitness_radius >= 0.0)) return fail(h, name + ": fitness_radius must be >= 0");
  if (q->stage_points != 0 && (q->stage_points < 16 || q->stage_points > kGoStage || q->stage_points % 16))
    return fail(h, name + ": stage_points must be 0 or a multiple of 16 in [16, " + std::to_string(kGoStage) + "]");
  return 0;
}

// what all nodes of `level` share, from the parameters alone
GoLevel go_level(const alignnet_goicp_params& q, int level, const int depth[4])
{
  GoLevel lv{};
  const double half[4] = {q.yaw_half, q.t_half[0], q.t_half[1], q.t_half[2]}, res[4] = {q.yaw_res, q.t_res, q.t_res, q.t_res};
  lv.level = level; lv.nchild = 1;
  for (int k = 0; k < 4; ++k) {
    lv.depth[k] = depth[k];
    lv.w[k] = std::ldexp(half[k], -depth[k]);
    lv.split[k] = lv.w[k] > res[k] ? 1 : 0;
    if (lv.split[k]) lv.nchild *= 2;
  }
  lv.gs = 2.0 * std::sin(std::min(lv.w[0], kGoPi) / 2.0);
  lv.an = std::sqrt(lv.w[1] * lv.w[1] + lv.w[2] * lv.w[2] + lv.w[3] * lv.w[3]);
  return lv;
}

// one evaluation launch over P pairs whose largest frontier is maxcount
int go_launch_eval(alignnet_handle* h, const GoArgs& a, const GoLevel& lv, int P, int maxcount, int cap, const int* nodes, const double* poses,
                   const int* count, double* ub, double* lb, double* fit = nullptr)
{
  if (maxcount < 1) return 0;
  if (maxcount > cap) return fail(h, "goicp: a frontier beyond its buffer");
  GoEval e{};
  e.sc = a.sc; e.qc = a.qc; e.ns = a.ns; e.nq = a.nq; e.nodes = nodes; e.poses = poses; e.count = count; e.ub = ub; e.lb = lb; e.fit = fit; e.fit_radius = a.prm.fitness_radius;
  e.ms = a.ms; e.mt = a.mt; e.cap = cap; e.stage = a.stage; e.trunc = a.prm.trunc; e.lv = lv;
  // a workgroup's share: one node per wave until the chip is covered, then more per workgroup (a batch of one pair spreads its frontier all the same)
  const long long total = (long long)maxcount * P;
  e.rounds = (int)std::max<long long>(1, (total + (long long)kGoWaves * kGoTargetWgs - 1) / ((long long)kGoWaves * kGoTargetWgs));
  e.npw = e.rounds * kGoWaves;
  const int gx = (maxcount + e.npw - 1) / e.npw;
  static alignnet::PerDeviceOnce attr;
  if (attr.need(h->cfg.device)) {
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(goicp_eval_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kGoStage * 32));
    attr.mark(h->cfg.device);
  }
  hipLaunchKernelGGL(goicp_eval_kernel, dim3(gx, P), dim3(kGoThreads), (size_t)a.stage * 32, h->stream, e);
  HIP_TRY(h, hipGetLastError());
  return 0;
}

struct GoDebug { const int32_t* depth; const int32_t* coords; int32_t K; double* ub; double* lb; };

struct GoOut { double* T; double* error; double* lower; double* fitness; int32_t* status; int32_t* evaluated; int32_t* survived; };

// shared driver: blobs and offsets on the device already; n1 / n2 = the cloud sizes of the B pairs (host)
int run_goicp(alignnet_handle* h, const std::string& name, const float* d_p0, const float* d_p1, const long long* d_off, const int* rows,
              const std::vector<long long>& n1, const std::vector<long long>& n2, int B, const alignnet_goicp_params& q, const GoOut& out,
              const GoDebug* dbg)
{
  GoArgs a{};
  a.prm = q; a.ms = q.max_source; a.mt = q.max_target; a.starts = dbg ? 0 : q.starts;
  a.cap = dbg ? std::max(dbg->K, 1) : q.max_frontier;
  // the sizes of this call's working sets shrink the stage arrays below max_source / max_target
  long long big1 = 1, big2 = 1;
  for (int i = 0; i < B; ++i) { big1 = std::max(big1, std::min<long long>(n1[i], q.max_source)); big2 = std::max(big2, std::min<long long>(n2[i], q.max_target)); }
  a.ms = (int)big1; a.mt = (int)big2;
  a.stage = q.stage_points ? q.stage_points : kGoStage;
  a.stage = std::min(a.stage, (a.mt + 15) & ~15);
  const size_t per_pair = go_carve(a, nullptr, 1);
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, kGoBudget / per_pair));
  const size_t need = go_carve(a, nullptr, chunk) + go_up((size_t)chunk * sizeof(int));
  if (grow_bytes(h, &h->goicp_ws, &h->goicp_ws_bytes, need)) return 1;
  const size_t used = go_carve(a, static_cast<char*>(h->goicp_ws), chunk);
  int* d_rows = reinterpret_cast<int*>(static_cast<char*>(h->goicp_ws) + used);
  a.pts[0] = d_p0; a.pts[1] = d_p1; a.off = d_off;
  std::vector<long long> h_wsoff((size_t)(chunk + 1) * 2), h_sn2, h_icp_wsoff;
  std::vector<int> h_count(chunk);
  for (int s = 0; s < B; s += chunk) {
    const int P = std::min(chunk, B - s);
    a.pair0 = 0; a.rows = nullptr;
    if (rows) { HIP_TRY(h, hipMemcpyAsync(d_rows, rows + s, (size_t)P * sizeof(int), hipMemcpyHostToDevice, h->stream)); a.rows = d_rows; }
    else a.pair0 = s;
    h_wsoff[0] = h_wsoff[1] = 0;
    for (int i = 0; i < P; ++i) {
      h_wsoff[(size_t)(i + 1) * 2] = h_wsoff[(size_t)i * 2] + std::min<long long>(n1[s + i], a.ms);
      h_wsoff[(size_t)(i + 1) * 2 + 1] = h_wsoff[(size_t)i * 2 + 1] + std::min<long long>(n2[s + i], a.mt);
    }
    HIP_TRY(h, hipMemcpyAsync(a.wsoff, h_wsoff.data(), (size_t)(P + 1) * 2 * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(goicp_prep_kernel, dim3(P, 2), dim3(256), 0, h->stream, a);
    hipLaunchKernelGGL(goicp_init_kernel, dim3((P + 63) / 64), dim3(64), 0, h->stream, a, P);
    HIP_TRY(h, hipGetLastError());
    int depth[4] = {0, 0, 0, 0};
    if (dbg) {   // one pair: K given nodes at the given depths, evaluated by the search's own launch
      for (int k = 0; k < 4; ++k) depth[k] = dbg->depth[k];
      const GoLevel lv = go_level(q, 0, depth);
      bool empty = n1[0] == 0 || n2[0] == 0;
      if (empty) return fail(h, name + ": an empty cloud has no bounds");
      HIP_TRY(h, hipMemcpyAsync(a.nodes[0], dbg->coords, (size_t)dbg->K * 4 * sizeof(int), hipMemcpyHostToDevice, h->stream));
      HIP_TRY(h, hipMemcpyAsync(a.count, &dbg->K, sizeof(int), hipMemcpyHostToDevice, h->stream));
      if (go_launch_eval(h, a, lv, 1, dbg->K, a.cap, a.nodes[0], nullptr, a.count, a.ub, a.lb)) return 1;
      HIP_TRY(h, hipMemcpyAsync(dbg->ub, a.ub, (size_t)dbg->K * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipMemcpyAsync(dbg->lb, a.lb, (size_t)dbg->K * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      return 0;
    }
    if (a.starts > 0) {   // the initial bound: `starts` z-constrained point-to-point ICP runs per pair on the working sets
      const int n = P * a.starts;
      h_sn2.resize(n);
      for (int b = 0; b < n; ++b) h_sn2[b] = std::min<long long>(n2[s + b / a.starts], a.mt);
      const long long stage_n2 = 0;   // the scan's LDS stage at its budget whatever the batch holds, as the _dataset entry points size it
      const alignnet::IcpDeviceIo io = {a.s_init, a.s_out, a.s_fit, a.s_rmse, a.s_iters, a.s_wsoff, &h_icp_wsoff};
      const float* const wpts[2] = {a.ws[0], a.ws[1]};
      if (alignnet_icp_run_device(h, wpts, a.wsoff, a.s_rows, nullptr, h_sn2.data(), stage_n2, n, io, q.start_radius, 0.0, q.start_its, false, 1)) return 1;
      hipLaunchKernelGGL(goicp_start_pose_kernel, dim3((n + 63) / 64), dim3(64), 0, h->stream, a, n);
      HIP_TRY(h, hipGetLastError());
      const GoLevel lv0 = go_level(q, 0, depth);
      if (go_launch_eval(h, a, lv0, P, a.starts, a.starts, nullptr, a.s_pose, a.s_count, a.s_ub, a.s_lb)) return 1;
      hipLaunchKernelGGL(goicp_start_best_kernel, dim3((P + 63) / 64), dim3(64), 0, h->stream, a, P);
      HIP_TRY(h, hipGetLastError());
    }
    int maxcount = 1, src = 0;
    for (int level = 0; level < q.max_levels && maxcount > 0; ++level) {   // (the last level's expand stops every pair: LEVELS)
      const GoLevel lv = go_level(q, level, depth);
      if (go_launch_eval(h, a, lv, P, maxcount, a.cap, a.nodes[src], nullptr, a.count, a.ub, a.lb)) return 1;
      hipLaunchKernelGGL(goicp_best_kernel, dim3(P), dim3(256), 0, h->stream, a, lv, src);
      hipLaunchKernelGGL(goicp_expand_kernel, dim3(P), dim3(kGoExpThreads), 0, h->stream, a, lv, src);
      HIP_TRY(h, hipGetLastError());
      HIP_TRY(h, hipMemcpyAsync(h_count.data(), a.count, (size_t)P * sizeof(int), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));   // the round's one read-back: the frontier sizes
      maxcount = 0;
      for (int i = 0; i < P; ++i) maxcount = std::max(maxcount, h_count[i]);
      if (maxcount > q.max_frontier) return fail(h, name + ": a frontier beyond max_frontier");
      for (int k = 0; k < 4; ++k) depth[k] += lv.split[k];
      src ^= 1;
    }
    if (go_launch_eval(h, a, go_level(q, 0, depth), P, 1, 1, nullptr, a.pose, a.one, a.f_ub, a.f_lb, a.fitness)) return 1;   // the fitness at the returned pose
    hipLaunchKernelGGL(goicp_finish_kernel, dim3((P + 63) / 64), dim3(64), 0, h->stream, a, P);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out.T + (size_t)s * 16, a.out_T, (size_t)P * 16 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (out.error) HIP_TRY(h, hipMemcpyAsync(out.error + s, a.best, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (out.lower) HIP_TRY(h, hipMemcpyAsync(out.lower + s, a.lower, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (out.fitness) HIP_TRY(h, hipMemcpyAsync(out.fitness + s, a.fitness, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (out.status) HIP_TRY(h, hipMemcpyAsync(out.status + s, a.status, (size_t)P * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (out.evaluated)
      HIP_TRY(h, hipMemcpyAsync(out.evaluated + (size_t)s * kGoLevels, a.evaluated, (size_t)P * kGoLevels * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (out.survived)
      HIP_TRY(h, hipMemcpyAsync(out.survived + (size_t)s * kGoLevels, a.survived, (size_t)P * kGoLevels * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // the next chunk reuses the arrays
  }
  return 0;
}

int goicp_host(alignnet_handle* h, const char* fn, const float* points1, const float* points2, const int64_t* offsets, int32_t B,
               const alignnet_goicp_params* params, const GoOut& out, const GoDebug* dbg)
{
  if (!h) return 1;
  const std::string name(fn);
  if (go_check_params(h, name, params)) return 1;
  if (!dbg && !out.T) return fail(h, name + ": null out_T");
  PairUpload u;
  if (upload_pairs(h, name, points1, points2, offsets, B, &u)) return 1;
  const int rc = run_goicp(h, name, u.pts[0].p, u.pts[1].p, u.off.p, nullptr, u.n1, u.n2, B, *params, out, dbg);
  hipStreamSynchronize(h->stream);   // before the uploaded clouds go
  return rc;
}

}  // namespace

extern "C" void alignnet_goicp_free(alignnet_handle* h)
{
  if (!h || !h->goicp_ws) return;
  hipFree(h->goicp_ws);
  h->goicp_ws = nullptr; h->goicp_ws_bytes = 0;
}

extern "C" int alignnet_goicp_register(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets, int32_t B,
                                       const alignnet_goicp_params* params, double* out_T, double* out_error, double* out_lower_bound,
                                       double* out_fitness, int32_t* out_status, int32_t* out_evaluated, int32_t* out_survived)
{
  return goicp_host(h, "alignnet_goicp_register", points1, points2, offsets, B, params,
                    GoOut{out_T, out_error, out_lower_bound, out_fitness, out_status, out_evaluated, out_survived}, nullptr);
}

extern "C" int alignnet_goicp_register_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, const alignnet_goicp_params* params,
                                               double* out_T, double* out_error, double* out_lower_bound, double* out_fitness,
                                               int32_t* out_status, int32_t* out_evaluated, int32_t* out_survived)
{
  if (!h) return 1;
  const std::string name("alignnet_goicp_register_dataset");
  if (go_check_params(h, name, params)) return 1;
  if (!out_T) return fail(h, name + ": null out_T");
  alignnet::DatasetTables t;
  if (!alignnet_dataset_tables(h, &t)) return fail(h, name + ": no dataset uploaded");
  if (!rows || B < 1) return fail(h, name + ": null rows or B < 1");
  for (int i = 0; i < B; ++i)
    if (rows[i] < 0 || rows[i] >= t.n) return fail(h, name + ": row " + std::to_string(rows[i]) + " out of range");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  std::vector<long long> n1(B), n2(B);
  for (int i = 0; i < B; ++i) {
    n1[i] = t.h_off[((size_t)rows[i] + 1) * 2] - t.h_off[(size_t)rows[i] * 2];
    n2[i] = t.h_off[((size_t)rows[i] + 1) * 2 + 1] - t.h_off[(size_t)rows[i] * 2 + 1];
  }
  return run_goicp(h, name, t.pts[0], t.pts[1], t.off, rows, n1, n2, B, *params,
                   GoOut{out_T, out_error, out_lower_bound, out_fitness, out_status, out_evaluated, out_survived}, nullptr);
}

extern "C" int alignnet_debug_goicp_nodes(alignnet_handle* h, const float* points1, int64_t n1, const float* points2, int64_t n2,
                                          const alignnet_goicp_params* params, const int32_t* depth, const int32_t* coords, int32_t K,
                                          double* ub, double* lb)
{
  if (!h) return 1;
  const std::string name("alignnet_debug_goicp_nodes");
  if (n1 < 0 || n2 < 0 || !depth || !coords || !ub || !lb || K < 1 || K > (1 << 24)) return fail(h, name + ": null argument, negative size or K outside [1, 2^24]");
  for (int k = 0; k < 4; ++k)
    if (depth[k] < 0 || depth[k] > kGoLevels) return fail(h, name + ": depth outside [0, " + std::to_string(kGoLevels) + "]");
  for (int64_t i = 0; i < (int64_t)K * 4; ++i)
    if (coords[i] < 0 || coords[i] >= (1 << depth[i & 3])) return fail(h, name + ": a coordinate outside [0, 2^depth)");
  const int64_t offsets[4] = {0, 0, n1, n2};
  const GoDebug dbg{depth, coords, K, ub, lb};
  return goicp_host(h, "alignnet_debug_goicp_nodes", points1, points2, offsets, 1, params, GoOut{}, &dbg);
}
