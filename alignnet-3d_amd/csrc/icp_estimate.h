// The 3x3 fp64 routines shared by ICP (alignnet_icp.hip) and the global registration (alignnet_globalreg.hip): the Umeyama rotation of the
// point-to-point estimates and the eigenvector behind both units' normals.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

// R = U diag(1, 1, sign(det U det V)) V^T for A = U S V^T (singular values descending): Eigen::umeyama's rotation without scaling, A = the
// centred cross-covariance sum (q - mean q)(p - mean p)^T (its 1 / n does not change U, V).  One-sided Jacobi on the columns of A (A V -> U S),
// fp64, one lane.  U is completed to a right-handed frame (u2 = u0 x u1; the sign fix then reads det V alone -- the same R, and no division by
// the smallest singular value), and u1 is Gram-Schmidt'ed against u0 (or chosen orthogonal to it when A has rank <= 1: collinear or coincident
// correspondences), so R is a finite proper rotation for every A.  The 3x3 matrices live in LDS (`work`, 27 doubles): held in registers
// they made this one-lane step spill 6 VGPRs instead of 4 (the scan with 17 sums alone compiles spill-free).
// In: work[0..8] = A (row-major).  Out: work[18..26] = R (row-major).
__device__ __forceinline__ void icp_umeyama_rotation(double* work)
{
  double* a = work;       // columns -> U S
  double* v = work + 9;   // columns -> V
  double* R = work + 18;
#pragma unroll
  for (int i = 0; i < 9; ++i) v[i] = i % 4 == 0 ? 1.0 : 0.0;
#pragma unroll 1
  for (int sweep = 0; sweep < 24; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int pr = 0; pr < 3; ++pr) {
      const int p = pr == 2 ? 1 : 0, q = pr == 0 ? 1 : 2;
      double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) { al += a[i * 3 + p] * a[i * 3 + p]; be += a[i * 3 + q] * a[i * 3 + q]; ga += a[i * 3 + p] * a[i * 3 + q]; }
      if (!(fabs(ga) > 1e-15 * sqrt(al * be))) continue;   // columns orthogonal to working precision (or one of them zero)
      const double ze = (be - al) / (2.0 * ga);
      const double t = (ze >= 0.0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(1.0 + ze * ze));
      const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double ap = a[i * 3 + p], aq = a[i * 3 + q], vp = v[i * 3 + p], vq = v[i * 3 + q];
        a[i * 3 + p] = c * ap - s * aq; a[i * 3 + q] = s * ap + c * aq;
        v[i * 3 + p] = c * vp - s * vq; v[i * 3 + q] = s * vp + c * vq;
      }
      rotated = true;
    }
    if (!rotated) break;
  }
  double sv[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) sv[k] = a[k] * a[k] + a[3 + k] * a[3 + k] + a[6 + k] * a[6 + k];
  // singular values descending (the sign fix acts on the smallest): compare-exchange of the column pairs (0,1), (1,2), (0,1)
#pragma unroll
  for (int pr = 0; pr < 3; ++pr) {
    const int p = pr == 1 ? 1 : 0, q = p + 1;
    if (sv[q] > sv[p]) {
      const double w = sv[p]; sv[p] = sv[q]; sv[q] = w;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double x = a[i * 3 + p]; a[i * 3 + p] = a[i * 3 + q]; a[i * 3 + q] = x;
        const double y = v[i * 3 + p]; v[i * 3 + p] = v[i * 3 + q]; v[i * 3 + q] = y;
      }
    }
  }
  double u0[3] = {1.0, 0.0, 0.0}, u1[3];
  const double s0 = sqrt(sv[0]);
  if (s0 > 1e-250)
    for (int i = 0; i < 3; ++i) u0[i] = a[i * 3] / s0;
  const double d01 = u0[0] * a[1] + u0[1] * a[4] + u0[2] * a[7];
  for (int i = 0; i < 3; ++i) u1[i] = a[i * 3 + 1] - d01 * u0[i];
  double n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
  if (!(n1 > 1e-250 + 1e-300 * s0)) {   // rank <= 1: any unit vector orthogonal to u0 (the axis u0 is least aligned with, minus its u0 part)
    const int k = fabs(u0[0]) <= fabs(u0[1]) ? (fabs(u0[0]) <= fabs(u0[2]) ? 0 : 2) : (fabs(u0[1]) <= fabs(u0[2]) ? 1 : 2);
    for (int i = 0; i < 3; ++i) u1[i] = (i == k ? 1.0 : 0.0) - u0[k] * u0[i];
    n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
  }
  for (int i = 0; i < 3; ++i) u1[i] /= n1;
  const double u2[3] = {u0[1] * u1[2] - u0[2] * u1[1], u0[2] * u1[0] - u0[0] * u1[2], u0[0] * u1[1] - u0[1] * u1[0]};
  const double detv = v[0] * (v[4] * v[8] - v[5] * v[7]) - v[1] * (v[3] * v[8] - v[5] * v[6]) + v[2] * (v[3] * v[7] - v[4] * v[6]);
  const double d = detv < 0.0 ? -1.0 : 1.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = u0[i] * v[j * 3] + u1[i] * v[j * 3 + 1] + d * u2[i] * v[j * 3 + 2];
}

// eigenvector of the smallest eigenvalue of the symmetric 3x3 matrix (a00, a01, a02, a11, a12, a22): cyclic Jacobi, fp64 (the normals of
// point-to-plane ICP and of the global registration)
__device__ __forceinline__ void icp_smallest_eigenvector(double a00, double a01, double a02, double a11, double a12, double a22, double* n)
{
  double A[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}};
  double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll 1
  for (int sweep = 0; sweep < 32; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int pr = 0; pr < 3; ++pr) {
      const int p = pr == 2 ? 1 : 0, q = pr == 0 ? 1 : 2;
      const double apq = A[p][q];
      if (!(fabs(apq) > 1e-18 * (fabs(A[p][p]) + fabs(A[q][q])))) continue;
      const double th = (A[q][q] - A[p][p]) / (2.0 * apq);
      const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(1.0 + th * th));
      const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
      const int r = 3 - p - q;
      const double arp = A[r][p], arq = A[r][q];
      A[p][p] -= t * apq; A[q][q] += t * apq; A[p][q] = 0.0; A[q][p] = 0.0;
      A[r][p] = cs * arp - sn * arq; A[p][r] = A[r][p];
      A[r][q] = sn * arp + cs * arq; A[q][r] = A[r][q];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double vp = V[i][p], vq = V[i][q];
        V[i][p] = cs * vp - sn * vq; V[i][q] = sn * vp + cs * vq;
      }
      rotated = true;
    }
    if (!rotated) break;
  }
  const double e0 = A[0][0], e1 = A[1][1], e2 = A[2][2];
  if (e0 <= e1 && e0 <= e2) { n[0] = V[0][0]; n[1] = V[1][0]; n[2] = V[2][0]; }
  else if (e1 <= e2) { n[0] = V[0][1]; n[1] = V[1][1]; n[2] = V[2][1]; }
  else { n[0] = V[0][2]; n[1] = V[1][2]; n[2] = V[2][2]; }
}
