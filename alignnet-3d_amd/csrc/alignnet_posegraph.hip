// Multiway registration: pose-graph optimisation of many small graphs at once (Choi, Zhou, Koltun 2015, as Open3D's global_optimization uses it:
// Levenberg-Marquardt, a line process on the uncertain edges in closed form), gfx950 only.  The computation is DEFINED by tests/pose_graph_ref.py,
// whose header states the graph, the residual, the objective, the Jacobians, the tied nodes and the loop; this file follows it decision by decision.
// Everything is fp64.
//
// pose_graph_kernel<kFull>: ONE WORKGROUP PER GRAPH (256 threads), one launch per chunk of graphs, the whole Levenberg-Marquardt loop inside it -- the
// accept / reject decision and the stop tests are taken from values every thread reads from LDS, so the control flow is uniform and nothing returns
// to the host between solves.  Stages of one linearisation:
//   edges     one thread per edge: D = X_j^-1 X_i T^-1, the residual, chi2, the weight l and the edge's term of F; when linearising also the
//             record the Jacobians are built from (R_j^T, a_i, a_j: 15 doubles) and r
//   assemble  one thread per (node, row, column) of the node's diagonal block, and one per (node, row) of b.  A thread walks the node's incident
//             edges IN EDGE ORDER (adjacency lists the host builds), keeps the diagonal entry in a register and adds the entry of the block
//             (node, other node) for other < node into the band -- an entry has ONE owner and a fixed order of additions: no atomics, and the
//             bits of a graph do not depend on what else is in the batch
//   solve     H is a symmetric band stored by columns: entry (row, col), row >= col, at col (bw + 1) + (row - col), half-bandwidth
//             bw = d (1 + max|i - j|) - 1.  (H + lambda I) is copied into a second band and factored there by a right-looking banded Cholesky (per
//             column: the pivot, the scaled column, the rank-one update of the (bw x bw) trailing triangle, each entry by one thread), then the
//             two triangular solves, column-oriented, one barrier per column.  A rejected step solves again from the kept H with another lambda.
//   trial     one thread per node: X_k <- rigid_about(p_k, dw, dv) X_k (as R <- rot3(dw) R, t <- t + dv) into the trial poses; edges again (chi2 and F only); F, x^T (lambda x - b) and
//             max|x| by fixed trees.
// Both bands, b and x form ONE region that lies in LDS when it fits kPgLdsDoubles (option "pose_graph_lds_budget") and in the graph's slice of the
// workspace otherwise; the solver takes a generic pointer and is the same code for both, so both placements give the same bits.  Per-edge and
// per-node working arrays always lie in the workspace.  Every loop is bounded by the graph's sizes or by max_solves; the host has checked every
// index before the launch.
#include "engine.h"
#include "host_util.h"
#include <cmath>
#include <numeric>
#include <vector>

namespace {

constexpr int kPgThreads = 256;
constexpr int kPgLdsDoubles = 20000;              // both bands + b + x of a graph in LDS: 156.25 KiB, beside 2 KiB of reduction scratch
constexpr size_t kPgRedBytes = kPgThreads * sizeof(double);
constexpr size_t kPgBudget = (size_t)1 << 30;     // working arrays of one chunk of graphs
constexpr int kPgMaxNodes = 1 << 20;

struct PgGraph {
  long long node0, edge0;    // the graph's rows of the concatenated node / edge arrays
  long long adj0;            // its n + 1 entries of adj_off
  long long work0;           // its working arrays, in doubles from PgArgs::work
  long long band0;           // its band region likewise, or -1: in LDS
  int n, m, bw1, pad;        // bw1 = half-bandwidth + 1
  double mu;
};

struct PgArgs {
  const double* poses; const int* edges; const double* T; const double* info; const double* c; const int* unc;   // the call's graphs, concatenated
  const int* tied;           // [nodes] 1: a chain of edges joins the node to node 0 of its graph
  const long long* adj_off;  // [nodes + G] per graph n + 1 offsets into adj
  const int* adj;            // incident edges of the tied nodes k >= 1, in edge order: 2 e + (1 when the node is the edge's j)
  const PgGraph* graphs;
  double* out_poses; double* before; double* after; int* solves; int* status; double* chi2; double* l;
  double* work;
  int g0, max_solves, debug;
};

__device__ inline double pg_block_sum(double v, double* red, int tid)
{
  red[tid] = v;
  __syncthreads();
  for (int s = kPgThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__device__ inline double pg_block_max(double v, double* red, int tid)
{
  red[tid] = v;
  __syncthreads();
  for (int s = kPgThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// sum of v[0 .. n) in a fixed order: thread t takes t, t + 256, ... in turn, then the tree
__device__ inline double pg_sum_array(const double* v, int n, double* red, int tid)
{
  double s = 0.0;
  for (int e = tid; e < n; e += kPgThreads) s += v[e];
  return pg_block_sum(s, red, tid);
}

__device__ inline double pg_info(const double* L, int p, int q) { return p <= q ? L[p * 6 + q] : L[q * 6 + p]; }   // the upper triangle only

// one edge at the poses X [n][16]: chi2, weight and term of F; with lin the record (R_j^T [9], a_i [3], a_j [3]) and r [6] as well
template <bool kFull>
__device__ void pg_eval_edge(const PgArgs& a, const PgGraph& g, int e, const double* X, bool lin, double* rec, double* er, double* chi2t, double* lt,
                             double* fe)
{
  constexpr int O = kFull ? 0 : 2;
  const long long ge = g.edge0 + e;
  const int i = a.edges[ge * 2], j = a.edges[ge * 2 + 1];
  const double* Xi = X + (size_t)i * 16; const double* Xj = X + (size_t)j * 16; const double* T = a.T + ge * 16; const double* L = a.info + ge * 36;
  double Ri[3][3], Rj[3][3], RT[3][3], ti[3], tj[3], tT[3], c[3];
  for (int p = 0; p < 3; ++p) {
    for (int q = 0; q < 3; ++q) { Ri[p][q] = Xi[p * 4 + q]; Rj[p][q] = Xj[p * 4 + q]; RT[p][q] = T[p * 4 + q]; }
    ti[p] = Xi[p * 4 + 3]; tj[p] = Xj[p * 4 + 3]; tT[p] = T[p * 4 + 3]; c[p] = a.c[ge * 3 + p];
  }
  double u[3], M[3][3], RD[3][3], tD[3], tinv[3];
  for (int p = 0; p < 3; ++p) tinv[p] = -(RT[0][p] * tT[0] + RT[1][p] * tT[1] + RT[2][p] * tT[2]);
  for (int p = 0; p < 3; ++p) {
    for (int q = 0; q < 3; ++q) M[p][q] = Ri[p][0] * RT[q][0] + Ri[p][1] * RT[q][1] + Ri[p][2] * RT[q][2];   // R_i R_T^T
    u[p] = (Ri[p][0] * tinv[0] + Ri[p][1] * tinv[1] + Ri[p][2] * tinv[2]) + (ti[p] - tj[p]);
  }
  for (int p = 0; p < 3; ++p) {
    for (int q = 0; q < 3; ++q) RD[p][q] = Rj[0][p] * M[0][q] + Rj[1][p] * M[1][q] + Rj[2][p] * M[2][q];
    tD[p] = Rj[0][p] * u[0] + Rj[1][p] * u[1] + Rj[2][p] * u[2];
  }
  double r[6];
  r[0] = kFull ? atan2(RD[2][1], RD[2][2]) : 0.0;
  r[1] = kFull ? -asin(fmin(1.0, fmax(-1.0, RD[2][0]))) : 0.0;
  r[2] = atan2(RD[1][0], RD[0][0]);
  for (int p = 0; p < 3; ++p) r[3 + p] = (tD[p] - c[p]) + (RD[p][0] * c[0] + RD[p][1] * c[1] + RD[p][2] * c[2]);
  double chi2 = 0.0;
  for (int p = O; p < 6; ++p) {
    double w = 0.0;
    for (int q = O; q < 6; ++q) w += pg_info(L, p, q) * r[q];
    chi2 += r[p] * w;
  }
  double l = 1.0, f = chi2;
  if (a.unc[ge]) { const double s = g.mu / (g.mu + chi2); l = s * s; f = g.mu * chi2 / (g.mu + chi2); }
  chi2t[e] = chi2; lt[e] = l; fe[e] = f;
  if (lin) {
    double* rc = rec + (size_t)e * 16;
    for (int p = 0; p < 3; ++p) {
      for (int q = 0; q < 3; ++q) rc[p * 3 + q] = Rj[q][p];
      // a = c - X_j^-1 p for p = the translations of X_i and of X_j
      rc[9 + p] = c[p] - (Rj[0][p] * (ti[0] - tj[0]) + Rj[1][p] * (ti[1] - tj[1]) + Rj[2][p] * (ti[2] - tj[2]));
      rc[12 + p] = c[p];
    }
    rc[15] = 0.0;
    for (int p = 0; p < 6; ++p) er[(size_t)e * 6 + p] = r[p];
  }
}

// column `pa` (parameter order: rotation x y z, translation x y z) of A(X_j, p, c) from the edge's record; av = the a of that node
__device__ inline void pg_column(const double* rc, const double* av, int pa, double sign, double v[6])
{
  if (pa < 3) {
    const double t0 = rc[pa], t1 = rc[3 + pa], t2 = rc[6 + pa];
    v[0] = sign * t0; v[1] = sign * t1; v[2] = sign * t2;
    v[3] = sign * (t1 * av[2] - t2 * av[1]); v[4] = sign * (t2 * av[0] - t0 * av[2]); v[5] = sign * (t0 * av[1] - t1 * av[0]);   // -(a x t)
  } else {
    v[0] = v[1] = v[2] = 0.0;
    v[3] = sign * rc[pa - 3]; v[4] = sign * rc[3 + pa - 3]; v[5] = sign * rc[6 + pa - 3];
  }
}

template <bool kFull>
__device__ inline double pg_form(const double* L, const double va[6], const double vb[6])   // va^T L vb over the rows and columns in use
{
  constexpr int O = kFull ? 0 : 2;
  double s = 0.0;
  for (int p = O; p < 6; ++p) {
    double w = 0.0;
    for (int q = O; q < 6; ++q) w += pg_info(L, p, q) * vb[q];
    s += va[p] * w;
  }
  return s;
}

// H (band) and b at the poses the records were taken at; l = the edges' weights
template <bool kFull>
__device__ void pg_assemble(const PgArgs& a, const PgGraph& g, const double* rec, const double* er, const double* l, double* Hb, double* bv, int tid)
{
  constexpr int D = kFull ? 6 : 4, O = kFull ? 0 : 2, DU = D * D + D;
  const int N = D * (g.n - 1), bw1 = g.bw1;
  for (int idx = tid; idx < N * bw1; idx += kPgThreads) Hb[idx] = 0.0;
  __syncthreads();
  for (int item = tid; item < (g.n - 1) * DU; item += kPgThreads) {
    const int k = 1 + item / DU, q = item % DU;
    const long long t0 = a.adj_off[g.adj0 + k], t1 = a.adj_off[g.adj0 + k + 1];
    const bool isb = q >= D * D;
    const int ca = isb ? q - D * D : q / D, cb = isb ? 0 : q % D;
    double acc = 0.0;
    for (long long t = t0; t < t1; ++t) {
      const int code = a.adj[t], e = code >> 1, role = code & 1;
      const long long ge = g.edge0 + e;
      const int o = a.edges[ge * 2 + (role ? 0 : 1)];
      const double* rc = rec + (size_t)e * 16;
      const double* L = a.info + ge * 36;
      const double* avk = rc + (role ? 12 : 9);
      const double sk = role ? -1.0 : 1.0, le = l[e];
      double va[6], vb[6];
      pg_column(rc, avk, ca + O, sk, va);
      if (isb) {
        acc += le * pg_form<kFull>(L, va, er + (size_t)e * 6);
        continue;
      }
      pg_column(rc, avk, cb + O, sk, vb);
      acc += le * pg_form<kFull>(L, va, vb);
      if (o >= 1 && o < k) {
        pg_column(rc, rc + (role ? 9 : 12), cb + O, -sk, vb);
        const int row = D * (k - 1) + ca, col = D * (o - 1) + cb;
        Hb[(size_t)col * bw1 + (row - col)] += le * pg_form<kFull>(L, va, vb);
      }
    }
    const int row = D * (k - 1) + ca;
    if (isb) bv[row] = acc;
    else if (ca >= cb) { const int col = D * (k - 1) + cb; Hb[(size_t)col * bw1 + (row - col)] = acc; }
  }
  __syncthreads();
}

// Lb <- chol(Hb + lambda I) in place of the copy; false (in every thread) when a pivot is not > 0.  Band by columns: (row, col) at col bw1 + row - col
__device__ bool pg_factor(const double* Hb, double* Lb, int N, int bw1, double lambda, int tid)
{
  for (int idx = tid; idx < N * bw1; idx += kPgThreads) Lb[idx] = Hb[idx] + (idx % bw1 == 0 ? lambda : 0.0);
  __syncthreads();
  for (int j = 0; j < N; ++j) {
    const int cnt = min(bw1 - 1, N - 1 - j);
    double* col = Lb + (size_t)j * bw1;
    const double p = col[0];
    if (!(p > 0.0)) return false;   // every thread reads the same value: uniform
    const double sq = sqrt(p);
    for (int s = 1 + tid; s <= cnt; s += kPgThreads) col[s] = col[s] / sq;
    __syncthreads();
    if (tid == 0) col[0] = sq;      // nobody reads the pivot during the update
    for (int idx = tid; idx < cnt * cnt; idx += kPgThreads) {
      const int u = idx / cnt + 1, v = idx % cnt + 1;
      if (v >= u) Lb[(size_t)(j + u) * bw1 + (v - u)] -= col[v] * col[u];
    }
    __syncthreads();
  }
  return true;
}

// x <- -(L L^T)^-1 b.  Column-oriented both ways; the entry being eliminated is divided by its pivot only after the sweep, so no thread writes what
// the others read in the same step
__device__ void pg_solve(const double* Lb, const double* bv, double* xv, int N, int bw1, int tid)
{
  for (int q = tid; q < N; q += kPgThreads) xv[q] = -bv[q];
  __syncthreads();
  for (int j = 0; j < N; ++j) {
    const int cnt = min(bw1 - 1, N - 1 - j);
    const double* col = Lb + (size_t)j * bw1;
    const double yj = xv[j] / col[0];
    for (int s = 1 + tid; s <= cnt; s += kPgThreads) xv[j + s] -= col[s] * yj;
    __syncthreads();
  }
  for (int q = tid; q < N; q += kPgThreads) xv[q] = xv[q] / Lb[(size_t)q * bw1];
  __syncthreads();
  for (int i = N - 1; i >= 0; --i) {
    const int cnt = min(bw1 - 1, i);
    const double xi = xv[i] / Lb[(size_t)i * bw1];
    for (int s = 1 + tid; s <= cnt; s += kPgThreads) xv[i - s] -= Lb[(size_t)(i - s) * bw1 + s] * xi;
    __syncthreads();
  }
  for (int q = tid; q < N; q += kPgThreads) xv[q] = xv[q] / Lb[(size_t)q * bw1];
  __syncthreads();
}

// Xt[k] = rigid_about(p_k, dw, dv) X[k] for the tied nodes k >= 1, a copy for the others
template <bool kFull>
__device__ void pg_step_poses(const PgArgs& a, const PgGraph& g, const double* X, const double* xv, double* Xt, int tid)
{
  constexpr int D = kFull ? 6 : 4;
  for (int k = tid; k < g.n; k += kPgThreads) {
    const double* s = X + (size_t)k * 16;
    double* d = Xt + (size_t)k * 16;
    if (k == 0 || !a.tied[g.node0 + k]) {
      for (int q = 0; q < 16; ++q) d[q] = s[q];
      continue;
    }
    const double* x = xv + (size_t)D * (k - 1);
    const double wx = kFull ? x[0] : 0.0, wy = kFull ? x[1] : 0.0, wz = kFull ? x[2] : x[0];
    const double v[3] = {x[D - 3], x[D - 2], x[D - 1]};
    const double cx = cos(wx), sx = sin(wx), cy = cos(wy), sy = sin(wy), cz = cos(wz), sz = sin(wz);
    const double G[3][3] = {{cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx},
                            {sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx},
                            {-sy, cy * sx, cy * cx}};   // Rz Ry Rx
    // rigid_about about p = the pose's own translation is R <- G R, t <- t + v in exact arithmetic; evaluated so (the restatement's rule: no
    // cancellation of two terms of the size of t)
    for (int r = 0; r < 3; ++r) {
      for (int q = 0; q < 3; ++q) d[r * 4 + q] = G[r][0] * s[q] + G[r][1] * s[4 + q] + G[r][2] * s[8 + q];
      d[r * 4 + 3] = s[r * 4 + 3] + v[r];
    }
    d[12] = 0.0; d[13] = 0.0; d[14] = 0.0; d[15] = 1.0;
  }
}

template <bool kFull>
__global__ __launch_bounds__(kPgThreads) void pose_graph_kernel(PgArgs a)
{
  extern __shared__ __attribute__((aligned(16))) char pg_smem[];
  constexpr int D = kFull ? 6 : 4;
  double* red = reinterpret_cast<double*>(pg_smem);
  const int tid = threadIdx.x, gi = a.g0 + blockIdx.x;
  const PgGraph g = a.graphs[gi];
  const int n = g.n, m = g.m, N = D * (n - 1), bw1 = g.bw1;
  double* X = a.out_poses + g.node0 * 16;
  double* w = a.work + g.work0;
  double* Xt = w; w += (size_t)n * 16;
  double* rec = w; w += (size_t)m * 16;
  double* er = w; w += (size_t)m * 6;
  double* chi2t = w; w += m;
  double* lt = w; w += m;
  double* fe = w;
  double* region = g.band0 >= 0 ? a.work + g.band0 : reinterpret_cast<double*>(pg_smem + kPgRedBytes);
  double* Hb = region;
  double* Lb = Hb + (size_t)N * bw1;
  double* bv = Lb + (size_t)N * bw1;
  double* xv = bv + N;
  double* chi2 = a.chi2 + g.edge0;
  double* l = a.l + g.edge0;

  for (int q = tid; q < n * 16; q += kPgThreads) X[q] = a.poses[g.node0 * 16 + q];
  __syncthreads();
  for (int e = tid; e < m; e += kPgThreads) pg_eval_edge<kFull>(a, g, e, X, true, rec, er, chi2t, lt, fe);
  __syncthreads();
  for (int e = tid; e < m; e += kPgThreads) { chi2[e] = chi2t[e]; l[e] = lt[e]; }
  double F = pg_sum_array(fe, m, red, tid);
  int status = ALIGNNET_POSE_GRAPH_EMPTY, solves = 0;
  const double F0 = F;
  double lambda = 0.0;
  if (n > 1 && m > 0) {
    pg_assemble<kFull>(a, g, rec, er, l, Hb, bv, tid);
    double dmax = 0.0;
    for (int q = tid; q < N; q += kPgThreads) dmax = fmax(dmax, Hb[(size_t)q * bw1]);
    lambda = 1e-3 * pg_block_max(dmax, red, tid);
  }
  if (lambda > 0.0 && !a.debug) {
    double nu = 2.0;
    for (;;) {
      if (solves == a.max_solves) { status = ALIGNNET_POSE_GRAPH_ITERATIONS; break; }
      ++solves;
      bool accept = false;
      double Fn = 0.0, rho = 0.0, step = 0.0;
      if (pg_factor(Hb, Lb, N, bw1, lambda, tid)) {
        pg_solve(Lb, bv, xv, N, bw1, tid);
        pg_step_poses<kFull>(a, g, X, xv, Xt, tid);
        __syncthreads();
        for (int e = tid; e < m; e += kPgThreads) pg_eval_edge<kFull>(a, g, e, Xt, false, rec, er, chi2t, lt, fe);
        __syncthreads();
        Fn = pg_sum_array(fe, m, red, tid);
        double ds = 0.0, xm = 0.0;
        for (int q = tid; q < N; q += kPgThreads) { const double x = xv[q]; ds += x * (lambda * x - bv[q]); xm = fmax(xm, fabs(x)); }
        const double den = pg_block_sum(ds, red, tid);
        step = pg_block_max(xm, red, tid);
        rho = (F - Fn) / den;
        accept = den > 0.0 && rho > 0.0;
      } else {
        __syncthreads();   // (the factor's early way out: its threads left between two barriers)
      }
      if (accept) {
        for (int q = tid; q < n * 16; q += kPgThreads) X[q] = Xt[q];
        for (int e = tid; e < m; e += kPgThreads) { chi2[e] = chi2t[e]; l[e] = lt[e]; }
        const bool conv = step < 1e-9 || F - Fn <= 1e-12 * F;
        F = Fn;
        __syncthreads();
        if (conv) { status = ALIGNNET_POSE_GRAPH_CONVERGED; break; }
        const double c = 2.0 * rho - 1.0;
        lambda *= fmax(1.0 / 3.0, 1.0 - c * c * c);
        nu = 2.0;
        for (int e = tid; e < m; e += kPgThreads) pg_eval_edge<kFull>(a, g, e, X, true, rec, er, chi2t, lt, fe);
        __syncthreads();
        pg_assemble<kFull>(a, g, rec, er, l, Hb, bv, tid);
      } else {
        lambda *= nu;
        nu *= 2.0;
        if (lambda > 1e30) { status = ALIGNNET_POSE_GRAPH_STALLED; break; }
      }
    }
  }
  if (tid == 0) { a.before[gi] = F0; a.after[gi] = F; a.solves[gi] = solves; a.status[gi] = status; }
}

size_t pg_up(size_t b) { return (b + 255) & ~(size_t)255; }

struct PgIn {
  int32_t G; const int64_t* node_off; const int64_t* edge_off; const double* poses; const int32_t* edges; const double* T; const double* info;
  const double* c; const int32_t* unc; const double* mu; int32_t flags, max_solves;
};
struct PgOut { double* poses; double* before; double* after; int32_t* solves; int32_t* status; double* chi2; double* l; };
struct PgDebug { double* r; double* H; double* b; };

bool pg_finite(const double* v, size_t n) { for (size_t k = 0; k < n; ++k) if (!std::isfinite(v[k])) return false; return true; }

// everything is checked here, before anything reaches the device
int pg_check(alignnet_handle* h, const std::string& name, const PgIn& in)
{
  if (in.G < 1 || !in.node_off || !in.edge_off || !in.poses || !in.mu) return fail(h, name + ": null argument or no graph");
  if (in.flags & ~ALIGNNET_ICP_FULL_ROTATION) return fail(h, name + ": unknown flags");
  if (in.max_solves < 1) return fail(h, name + ": max_solves must be >= 1");
  if (in.node_off[0] != 0 || in.edge_off[0] != 0) return fail(h, name + ": offsets start at 0");
  for (int g = 0; g < in.G; ++g) {
    const int64_t n = in.node_off[g + 1] - in.node_off[g], m = in.edge_off[g + 1] - in.edge_off[g];
    const std::string where = name + ": graph " + std::to_string(g);
    if (n < 1 || n > kPgMaxNodes || m < 0 || m > (1 << 24)) return fail(h, where + ": 1 .. 2^20 nodes and 0 .. 2^24 edges");
    if (!(in.mu[g] > 0.0) || !std::isfinite(in.mu[g])) return fail(h, where + ": mu must be > 0 and finite");
    if (!pg_finite(in.poses + in.node_off[g] * 16, (size_t)n * 16)) return fail(h, where + ": a pose entry is not finite");
    if (m && (!in.edges || !in.T || !in.info || !in.c || !in.unc)) return fail(h, where + ": null edge array");
    for (int64_t e = in.edge_off[g]; e < in.edge_off[g + 1]; ++e) {
      const int i = in.edges[e * 2], j = in.edges[e * 2 + 1];
      if (i < 0 || i >= n || j < 0 || j >= n) return fail(h, where + ": edge index out of range");
      if (i == j) return fail(h, where + ": an edge joins a node to itself");
      if (!pg_finite(in.T + e * 16, 16) || !pg_finite(in.c + e * 3, 3)) return fail(h, where + ": a transform or centre entry is not finite");
      for (int p = 0; p < 6; ++p)
        for (int q = p; q < 6; ++q)
          if (!std::isfinite(in.info[e * 36 + p * 6 + q])) return fail(h, where + ": an information entry is not finite");
    }
  }
  return 0;
}

int run_pose_graph(alignnet_handle* h, const std::string& name, const PgIn& in, const PgOut& out, const PgDebug* dbg)
{
  if (pg_check(h, name, in)) return 1;
  if (!out.poses && !dbg) return fail(h, name + ": null out_poses");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  const bool full = (in.flags & ALIGNNET_ICP_FULL_ROTATION) != 0;
  const int D = full ? 6 : 4, G = in.G;
  const long long nodes = in.node_off[G], E = in.edge_off[G];
  const int lds_budget = dbg ? 0 : (h->pose_graph_lds_budget < 0 ? kPgLdsDoubles : h->pose_graph_lds_budget);

  // per graph: the tied nodes (union-find), the adjacency lists in edge order, the bandwidth, the working arrays
  std::vector<PgGraph> graphs(G);
  std::vector<int> tied((size_t)std::max<long long>(nodes, 1)), adj, root;
  std::vector<long long> adj_off((size_t)nodes + G);
  std::vector<size_t> work_doubles(G);
  int lds_graphs = 0;
  for (int g = 0; g < G; ++g) {
    const int n = (int)(in.node_off[g + 1] - in.node_off[g]), m = (int)(in.edge_off[g + 1] - in.edge_off[g]);
    const int32_t* ed = in.edges + in.edge_off[g] * 2;
    root.resize(n);
    std::iota(root.begin(), root.end(), 0);
    auto find = [&](int x) { while (root[x] != x) { root[x] = root[root[x]]; x = root[x]; } return x; };
    int gap = 0;
    for (int e = 0; e < m; ++e) {
      const int ra = find(ed[e * 2]), rb = find(ed[e * 2 + 1]);
      if (ra != rb) root[std::max(ra, rb)] = std::min(ra, rb);
      gap = std::max(gap, std::abs(ed[e * 2] - ed[e * 2 + 1]));
    }
    int* td = tied.data() + in.node_off[g];
    for (int k = 0; k < n; ++k) td[k] = find(k) == 0;
    // counting sort of the incident edges by node keeps the edge order inside a node's list
    long long* ao = adj_off.data() + in.node_off[g] + g;
    std::vector<int> cnt(n + 1, 0);
    for (int e = 0; e < m; ++e)
      for (int s = 0; s < 2; ++s) { const int k = ed[e * 2 + s]; if (k >= 1 && td[k]) ++cnt[k]; }
    const long long base = (long long)adj.size();
    ao[0] = base;
    for (int k = 0; k < n; ++k) ao[k + 1] = ao[k] + cnt[k];
    adj.resize((size_t)ao[n]);
    std::vector<long long> fill(ao, ao + n);
    for (int e = 0; e < m; ++e)
      for (int s = 0; s < 2; ++s) { const int k = ed[e * 2 + s]; if (k >= 1 && td[k]) adj[(size_t)fill[k]++] = e * 2 + s; }
    PgGraph& pg = graphs[g];
    pg.node0 = in.node_off[g]; pg.edge0 = in.edge_off[g]; pg.adj0 = in.node_off[g] + g; pg.n = n; pg.m = m; pg.pad = 0; pg.mu = in.mu[g];
    const long long N = (long long)D * (n - 1);
    pg.bw1 = (int)std::max<long long>(1, std::min<long long>(N, (long long)D * (1 + gap)));
    const size_t region = 2 * (size_t)N * pg.bw1 + 2 * (size_t)N;
    const bool in_lds = region <= (size_t)lds_budget;
    lds_graphs += in_lds && n > 1 && m > 0;
    pg.band0 = in_lds ? -1 : 0;   // (the offset follows with the chunks)
    work_doubles[g] = (size_t)n * 16 + (size_t)m * 25 + (in_lds ? 0 : region);
  }
  h->pose_graph_lds_graphs = lds_graphs;

  // chunks of graphs whose working arrays fit the budget (a graph that needs more forms a chunk alone)
  const size_t budget = h->pose_graph_ws_budget ? h->pose_graph_ws_budget : kPgBudget;
  std::vector<int> first;
  size_t cur = 0, big = 0;
  for (int g = 0; g < G; ++g) {
    const size_t bytes = pg_up(work_doubles[g] * sizeof(double));
    if (g == 0 || cur + bytes > budget || g - first.back() >= 65535) { first.push_back(g); cur = 0; }
    const size_t region = 2 * (size_t)D * (graphs[g].n - 1) * graphs[g].bw1 + 2 * (size_t)D * (graphs[g].n - 1);
    graphs[g].work0 = (long long)(cur / sizeof(double));
    if (graphs[g].band0 >= 0) graphs[g].band0 = graphs[g].work0 + (long long)(work_doubles[g] - region);
    cur += bytes;
    big = std::max(big, cur);
  }
  first.push_back(G);
  h->pose_graph_chunks = (int)first.size() - 1;

  // one workspace: inputs, results, tables, then the chunk's working arrays
  size_t off = 0;
  auto carve = [&](size_t bytes) { const size_t at = off; off += pg_up(std::max<size_t>(bytes, 8)); return at; };
  const size_t o_poses = carve((size_t)nodes * 16 * 8), o_edges = carve((size_t)E * 2 * 4), o_T = carve((size_t)E * 16 * 8), o_info = carve((size_t)E * 36 * 8),
               o_c = carve((size_t)E * 3 * 8), o_unc = carve((size_t)E * 4), o_tied = carve((size_t)nodes * 4), o_adjoff = carve(adj_off.size() * 8),
               o_adj = carve(adj.size() * 4), o_graphs = carve((size_t)G * sizeof(PgGraph)), o_out = carve((size_t)nodes * 16 * 8),
               o_before = carve((size_t)G * 8), o_after = carve((size_t)G * 8), o_solves = carve((size_t)G * 4), o_status = carve((size_t)G * 4),
               o_chi2 = carve((size_t)E * 8), o_l = carve((size_t)E * 8), o_work = carve(big);
  if (grow_bytes(h, &h->pose_graph_ws, &h->pose_graph_ws_bytes, off)) return 1;
  char* ws = static_cast<char*>(h->pose_graph_ws);
  auto up = [&](size_t at, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(ws + at, src, bytes, hipMemcpyHostToDevice, h->stream) : hipSuccess; };
  HIP_TRY(h, up(o_poses, in.poses, (size_t)nodes * 16 * 8));
  HIP_TRY(h, up(o_edges, in.edges, (size_t)E * 2 * 4));
  HIP_TRY(h, up(o_T, in.T, (size_t)E * 16 * 8));
  HIP_TRY(h, up(o_info, in.info, (size_t)E * 36 * 8));
  HIP_TRY(h, up(o_c, in.c, (size_t)E * 3 * 8));
  HIP_TRY(h, up(o_unc, in.unc, (size_t)E * 4));
  HIP_TRY(h, up(o_tied, tied.data(), (size_t)nodes * 4));
  HIP_TRY(h, up(o_adjoff, adj_off.data(), adj_off.size() * 8));
  HIP_TRY(h, up(o_adj, adj.data(), adj.size() * 4));
  HIP_TRY(h, up(o_graphs, graphs.data(), (size_t)G * sizeof(PgGraph)));
  PgArgs a{};
  a.poses = reinterpret_cast<const double*>(ws + o_poses); a.edges = reinterpret_cast<const int*>(ws + o_edges); a.T = reinterpret_cast<const double*>(ws + o_T);
  a.info = reinterpret_cast<const double*>(ws + o_info); a.c = reinterpret_cast<const double*>(ws + o_c); a.unc = reinterpret_cast<const int*>(ws + o_unc);
  a.tied = reinterpret_cast<const int*>(ws + o_tied); a.adj_off = reinterpret_cast<const long long*>(ws + o_adjoff); a.adj = reinterpret_cast<const int*>(ws + o_adj);
  a.graphs = reinterpret_cast<const PgGraph*>(ws + o_graphs); a.out_poses = reinterpret_cast<double*>(ws + o_out);
  a.before = reinterpret_cast<double*>(ws + o_before); a.after = reinterpret_cast<double*>(ws + o_after); a.solves = reinterpret_cast<int*>(ws + o_solves);
  a.status = reinterpret_cast<int*>(ws + o_status); a.chi2 = reinterpret_cast<double*>(ws + o_chi2); a.l = reinterpret_cast<double*>(ws + o_l);
  a.work = reinterpret_cast<double*>(ws + o_work); a.max_solves = in.max_solves; a.debug = dbg ? 1 : 0;

  static alignnet::PerDeviceOnce attr;
  if (attr.need(h->cfg.device)) {
    const int most = (int)(kPgRedBytes + (size_t)kPgLdsDoubles * sizeof(double));
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(pose_graph_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, most));
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(pose_graph_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, most));
    attr.mark(h->cfg.device);
  }
  for (size_t c = 0; c + 1 < first.size(); ++c) {
    const int lo = first[c], hi = first[c + 1];
    size_t lds = 0;   // the largest region of the chunk's graphs that lie in LDS
    for (int g = lo; g < hi; ++g)
      if (graphs[g].band0 < 0) lds = std::max(lds, (2 * (size_t)D * (graphs[g].n - 1) * graphs[g].bw1 + 2 * (size_t)D * (graphs[g].n - 1)) * sizeof(double));
    a.g0 = lo;
    alignnet::ProfScope prof_scope(h, alignnet::PK_POSE_GRAPH, true);
    if (full) TIMED_LAUNCH(pose_graph_kernel<true>, dim3(hi - lo), dim3(kPgThreads), kPgRedBytes + lds, a);
    else TIMED_LAUNCH(pose_graph_kernel<false>, dim3(hi - lo), dim3(kPgThreads), kPgRedBytes + lds, a);
    HIP_TRY(h, hipGetLastError());
    if (dbg) {   // one graph, its band in the workspace: r, the dense H and b from the kernel's own arrays
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      const PgGraph& pg = graphs[0];
      const int N = D * (pg.n - 1), O = full ? 0 : 2;
      std::vector<double> er((size_t)pg.m * 6), band((size_t)N * pg.bw1 + 1);
      const double* w = a.work + pg.work0;
      if (pg.m) HIP_TRY(h, hipMemcpy(er.data(), w + (size_t)pg.n * 16 + (size_t)pg.m * 16, er.size() * 8, hipMemcpyDeviceToHost));
      for (int e = 0; e < pg.m; ++e)
        for (int q = 0; q < D; ++q) dbg->r[(size_t)e * D + q] = er[(size_t)e * 6 + O + q];
      for (size_t q = 0; q < (size_t)N * N; ++q) dbg->H[q] = 0.0;
      for (int q = 0; q < N; ++q) dbg->b[q] = 0.0;
      if (pg.n > 1 && pg.m > 0) {
        HIP_TRY(h, hipMemcpy(band.data(), a.work + pg.band0, (size_t)N * pg.bw1 * 8, hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(dbg->b, a.work + pg.band0 + 2 * (size_t)N * pg.bw1, (size_t)N * 8, hipMemcpyDeviceToHost));
        for (int col = 0; col < N; ++col)
          for (int s = 0; s < pg.bw1 && col + s < N; ++s) dbg->H[(size_t)(col + s) * N + col] = dbg->H[(size_t)col * N + col + s] = band[(size_t)col * pg.bw1 + s];
      }
    }
    if (c + 2 < first.size()) HIP_TRY(h, hipStreamSynchronize(h->stream));   // the next chunk reuses the working arrays
  }
  auto down = [&](void* dst, size_t at, size_t bytes) { return dst && bytes ? hipMemcpyAsync(dst, ws + at, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess; };
  HIP_TRY(h, down(out.poses, o_out, (size_t)nodes * 16 * 8));
  HIP_TRY(h, down(out.before, o_before, (size_t)G * 8));
  HIP_TRY(h, down(out.after, o_after, (size_t)G * 8));
  HIP_TRY(h, down(out.solves, o_solves, (size_t)G * 4));
  HIP_TRY(h, down(out.status, o_status, (size_t)G * 4));
  HIP_TRY(h, down(out.chi2, o_chi2, (size_t)E * 8));
  HIP_TRY(h, down(out.l, o_l, (size_t)E * 8));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return 0;
}

}  // namespace

extern "C" void alignnet_posegraph_free(alignnet_handle* h)
{
  if (!h || !h->pose_graph_ws) return;
  hipFree(h->pose_graph_ws);
  h->pose_graph_ws = nullptr; h->pose_graph_ws_bytes = 0;
}

extern "C" int alignnet_pose_graph_optimize(alignnet_handle* h, int32_t G, const int64_t* node_offsets, const int64_t* edge_offsets, const double* poses,
                                            const int32_t* edges, const double* transforms, const double* informations, const double* centres,
                                            const int32_t* uncertain, const double* mu, int32_t flags, int32_t max_solves, double* out_poses,
                                            double* out_before, double* out_after, int32_t* out_solves, int32_t* out_status, double* out_chi2,
                                            double* out_weights)
{
  if (!h) return 1;
  const PgIn in{G, node_offsets, edge_offsets, poses, edges, transforms, informations, centres, uncertain, mu, flags, max_solves};
  return run_pose_graph(h, "alignnet_pose_graph_optimize", in, PgOut{out_poses, out_before, out_after, out_solves, out_status, out_chi2, out_weights}, nullptr);
}

extern "C" int alignnet_debug_pose_graph_system(alignnet_handle* h, int32_t n, int32_t m, const double* poses, const int32_t* edges, const double* transforms,
                                                const double* informations, const double* centres, const int32_t* uncertain, double mu, int32_t flags,
                                                double* r, double* chi2, double* weights, double* F, double* H, double* b)
{
  if (!h) return 1;
  if (!r || !chi2 || !weights || !F || !H || !b) return fail(h, "alignnet_debug_pose_graph_system: null result");
  const int64_t node_off[2] = {0, n}, edge_off[2] = {0, m};
  const PgIn in{1, node_off, edge_off, poses, edges, transforms, informations, centres, uncertain, &mu, flags, 1};
  const PgDebug dbg{r, H, b};
  return run_pose_graph(h, "alignnet_debug_pose_graph_system", in, PgOut{nullptr, F, nullptr, nullptr, nullptr, chi2, weights}, &dbg);
}
