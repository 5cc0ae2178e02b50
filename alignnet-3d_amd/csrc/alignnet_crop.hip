// KITTI tracklet extraction (the KITTITracklets* datasets of tp_utils/pointcloud.py:769-778, 840-869, 918-940, 1000-1033), gfx950 only.
//
// Replaces extract_pointcloud -> compute_box_3d -> extract_pc_in_box3d (scipy's Delaunay.find_simplex on the box's eight corners): the
// points of a LiDAR scan that lie in a tracked 3D box are kept in scan order.  The semantics are DEFINED by tests/tracklet_ref.py (fp64, NumPy):
//  - a scan point p = (x, y, z) float32 in the Velodyne frame has camera-frame coordinates q = (-y, -z, x) (the reference's R = R1 R2, a signed
//    permutation: exact);
//  - a box b = (bx, by, bz, h, w, l, ry) (the label's location, dimensions, rotation_y); d = q - (bx, by, bz) in fp64, c = cos ry, s = sin ry evaluated ONCE on
//    the host in fp64 and handed over, lx = c dx - s dz, ly = dy, lz = s dx + c dz, every product and difference rounded as written (no fused
//    multiply-add: bit for bit the restatement's numbers).  Inside iff |lx| <= l / 2, -h <= ly <= 0, |lz| <= w / 2: the box is CLOSED;
//  - a point with a non-finite coordinate is in no box;
//  - the crop keeps the points in scan order with their float32 bits unchanged (the reference's pc[inds]); dz is subtracted from z in ONE
//    float32 subtraction (pc2[:, 2] -= z_difference on a float32 array under the NumPy of the reference's time).  No colour columns.
//
// Stages of one extraction (B pairs = 2 B crop jobs against the uploaded scans); the host groups the jobs by frame.  The two kernels that test
// points are templates on a crop policy C (BoxCrop here, FrustumCrop below: the membership test and what it needs per job, frame and point) and
// on the scans' stride; everything else of them is written once:
//  1. crop_test_kernel<C>, one workgroup of four waves per (frame, chunk of kTrackletChunk points): the chunk's points are loaded once (stride 4:
//     one 16-byte load per point) and held in registers, four per thread, a wave holding 64 consecutive points per quarter; C::prepare then
//     derives what the policy keeps per point.  The frame's jobs go through LDS in passes of kTrackletJobsPerPass.  Per job and quarter
//     C::ballot gives the wave's membership mask; its popcount is the wave's count, the four waves' counts go to counts[job][chunk].
//     BoxCrop::ballot: a float32 pre-test, then (only where some lane of the wave passed it) the fp64 test.
//     The pre-test is CONSERVATIVE: with bf = float(b) and df = q (-) bf in float32, |df| <= (|d| + 2^-24 |b|)(1 + 2^-24); an inside point has
//     |dx|, |dz| <= hypot(l / 2, w / 2) and |dy| <= h, so a point is rejected only when |df| exceeds that bound enlarged by (|b| 6e-8) and a factor
//     1 + 1e-6, rounded up to the next float.  A NaN compares false and is never rejected here (the fp64 test refuses it).
//  2. tracklet_jobscan_kernel, one workgroup per job: the exclusive scan of the job's counts in chunk order -> the position of every (job, chunk)
//     inside the job's crop, and the job's total; tracklet_scan_kernel, one workgroup: the exclusive scan of the totals in pair order per cloud
//     index -> the offsets table [B + 1][2].  It goes to the host (the one small copy of a call), which sizes the blobs from its last row.
//  3. crop_scatter_kernel<C>, the grid of stage 1: a workgroup reads its chunk's counts of 64 jobs at once (a lane each) and skips every job whose
//     count is zero (typically under 2 % of a frame's points are in any box: most chunks load no point at all), repeats the test of stage 1
//     for the others (the same function on the same numbers) and writes the members at offsets[pair][cloud] + position + ballot prefix.
//     Counts, a scan, a scatter: no atomics that could reorder points.
// The result is built in a second pair of blobs and swapped in on success: an error leaves the previous result and the uploaded scans as they were.
//
// The image-frustum crop (extract_pointcloud with from_bbox2d: extract_pc_in_box2d -> get_lidar_in_image_fov -> project_velo_to_image,
// tp_utils/pointcloud.py:781-801, 41-202): every LiDAR return whose image projection falls inside the object's 2D box.  DEFINED by
// tests/frustum_ref.py (fp64, NumPy):
//  - a frame has a projection M [3][4] = P (R0 padded to 4 x 4) (V2C padded to 4 x 4), multiplied ONCE on the host in fp64 and handed over, an
//    image size (W, H) and the call a clip distance; a job has a rectangle (xmin, ymin, xmax, ymax);
//  - w_i = ((M[i][0] x + M[i][1] y) + M[i][2] z) + M[i][3] with x, y, z widened to fp64, every product and sum rounded as written (no fused
//    multiply-add); u = w_0 / w_2, v = w_1 / w_2 (IEEE fp64 divisions);
//  - the point is kept iff its coordinates are finite, x > clip, 0 <= u < W, 0 <= v < H, xmin <= u < xmax and ymin <= v < ymax: HALF-OPEN
//    intervals, the reference's.  A comparison with a NaN or infinite u / v is false (w_2 == 0 needs no special case); the sign of w_2 is not
//    tested (the reference's front test is x > clip);
//  - order, bits and dz as for the box crop.
// The calibration belongs to the FRAME: FrustumCrop::prepare projects each of a thread's four points ONCE (u, v and an "in the image and in
// front" flag: the two divisions are paid per chunk, not per job), and FrustumCrop::ballot is four fp64 compares on those registers.  There is
// no float32 pre-test.  alignnet_tracklet_extract_frustum shares everything else with alignnet_tracklet_extract (run_extract below).
#include "engine.h"
#include "host_util.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

namespace {

constexpr int kChunk = alignnet::kTrackletChunk, kJobsPerPass = alignnet::kTrackletJobsPerPass;
constexpr int kThreads = 256, kQuarters = kChunk / kThreads;
static_assert(kChunk % kThreads == 0 && kQuarters == 4, "a thread holds four points of a chunk");

struct CropJob {
  double bx, by, bz, c, s, hl, h, hw;   // box centre (camera frame), cos / sin of ry, l / 2, h, w / 2
  float fx, fy, fz, txz, ty, dz;        // float32 pre-test: centre, bounds on |dx|, |dz| and on |dy|; dz: subtracted from z
  long long cbase;                      // the job's first entry in the counts / positions tables
  int which, pair;                      // cloud index 0 / 1; the pair: the crop starts at offsets[pair][which]
};
static_assert(sizeof(CropJob) == 104, "LDS budget");

// first point of the frame in the uploaded scans, its points, its jobs in the sorted job list, its index in the upload (the frustum's calibration)
struct CropFrame { long long pt0; int n, job0, njobs, frame; };

struct Pt { float x, y, z; };

__device__ __forceinline__ bool crop_pre(const CropJob& j, const Pt& p)
{
  // q = (-y, -z, x); false = certainly outside (NaN: never rejected here)
  return !(fabsf(-p.y - j.fx) > j.txz) && !(fabsf(-p.z - j.fy) > j.ty) && !(fabsf(p.x - j.fz) > j.txz);
}

__device__ __forceinline__ bool crop_inside(const CropJob& j, const Pt& p)
{
#pragma clang fp contract(off)
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) return false;
  const double dx = (double)(-p.y) - j.bx, dy = (double)(-p.z) - j.by, dz = (double)p.x - j.bz;
  const double lx = j.c * dx - j.s * dz, lz = j.s * dx + j.c * dz;
  return fabs(lx) <= j.hl && -j.h <= dy && dy <= 0.0 && fabs(lz) <= j.hw;
}

// A crop policy C is what crop_test_kernel and crop_scatter_kernel are compiled for (static functions only: nothing is chosen at run time):
//  - C::Job, a job as the kernels read it (dz, cbase, which, pair and what the test needs); C::Cal, what the test needs per frame (void: nothing);
//  - C::Prep, what a thread keeps per point besides the point; C::prepare fills it for the thread's kQuarters points, once per chunk;
//  - C::ballot, the membership of the wave's 64 points of one quarter in one job.
struct BoxCrop {
  typedef CropJob Job;
  typedef void Cal;
  typedef bool Prep;   // the point exists (the chunk's tail)
  static __device__ __forceinline__ void prepare(const Cal*, const CropFrame&, const Pt*, const bool* valid, Prep* q)
  {
#pragma unroll
    for (int i = 0; i < kQuarters; ++i) q[i] = valid[i];
  }
  // the pre-test first, the fp64 test only where some lane passed it
  static __device__ __forceinline__ unsigned long long ballot(const Job& j, const Pt& p, const Prep& valid)
  {
    const bool pre = valid && crop_pre(j, p);
    if (__ballot(pre) == 0ull) return 0ull;
    return __ballot(pre && crop_inside(j, p));
  }
};

template <int STRIDE>
__device__ __forceinline__ void load_points(const float* __restrict__ scans, const CropFrame& f, int chunk, Pt* p, bool* valid)
{
#pragma unroll
  for (int i = 0; i < kQuarters; ++i) {
    const int k = chunk * kChunk + i * kThreads + (int)threadIdx.x;   // a wave holds 64 consecutive points of quarter i
    valid[i] = k < f.n;
    p[i].x = p[i].y = p[i].z = 0.f;
    if (valid[i]) {
      const long long e = f.pt0 + k;
      if (STRIDE == 4) {
        const float4 v = *reinterpret_cast<const float4*>(scans + e * 4);   // the scans' base is an allocation's: 16-byte aligned
        p[i].x = v.x; p[i].y = v.y; p[i].z = v.z;
      } else {
        p[i].x = scans[e * 3]; p[i].y = scans[e * 3 + 1]; p[i].z = scans[e * 3 + 2];
      }
    }
  }
}

// grid: the (frame, chunk) items
template <class C, int STRIDE>
__global__ __launch_bounds__(kThreads) void crop_test_kernel(const float* __restrict__ scans, const CropFrame* __restrict__ frames,
                                                             const int2* __restrict__ items, const typename C::Job* __restrict__ jobs,
                                                             const typename C::Cal* __restrict__ cals, int* __restrict__ counts)
{
  typedef typename C::Job Job;
  static_assert(sizeof(Job) % 4 == 0, "jobs are staged dword by dword");
  __shared__ Job sj[kJobsPerPass];
  __shared__ int wcnt[kJobsPerPass][4];
  const int2 it = items[blockIdx.x];
  const CropFrame f = frames[it.x];
  const int chunk = it.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  Pt p[kQuarters]; typename C::Prep q[kQuarters];
  {
    bool valid[kQuarters];
    load_points<STRIDE>(scans, f, chunk, p, valid);
    C::prepare(cals, f, p, valid, q);
  }
  for (int j0 = 0; j0 < f.njobs; j0 += kJobsPerPass) {
    const int nj = min(kJobsPerPass, f.njobs - j0);
    {
      // stage the pass's jobs, dword by dword
      const int* src = reinterpret_cast<const int*>(jobs + f.job0 + j0);
      int* dst = reinterpret_cast<int*>(sj);
      for (int e = tid; e < nj * (int)(sizeof(Job) / 4); e += kThreads) dst[e] = src[e];
    }
    __syncthreads();
    for (int j = 0; j < nj; ++j) {
      int n = 0;
#pragma unroll
      for (int i = 0; i < kQuarters; ++i) n += __popcll(C::ballot(sj[j], p[i], q[i]));
      if (lane == 0) wcnt[j][wave] = n;
    }
    __syncthreads();
    for (int j = tid; j < nj; j += kThreads) counts[sj[j].cbase + chunk] = wcnt[j][0] + wcnt[j][1] + wcnt[j][2] + wcnt[j][3];
    __syncthreads();
  }
}

struct JobSpan { long long cbase; int chunks, pad; };   // a job's entries in the counts / positions tables, in (pair, cloud) order

// grid: the 2 B jobs in (pair, cloud) order.  pos[entry] = members of the job in earlier chunks; total[job]
__global__ __launch_bounds__(kThreads) void tracklet_jobscan_kernel(const int* __restrict__ counts, const JobSpan* __restrict__ spans, int* __restrict__ pos,
                                                                    int* __restrict__ total)
{
  __shared__ int wsum[4];
  const JobSpan sp = spans[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int run = 0;   // members in the chunks before this tile of 256 (the same in every thread)
  for (int e0 = 0; e0 < sp.chunks; e0 += kThreads) {
    const int e = e0 + tid;
    const int v = e < sp.chunks ? counts[sp.cbase + e] : 0;
    int inc = v;   // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = run, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const int n = wsum[w]; if (w < wave) before += n; all += n; }
    if (e < sp.chunks) pos[sp.cbase + e] = before + inc - v;
    run += all;
    __syncthreads();
  }
  if (tid == 0) total[blockIdx.x] = run;
}

// one workgroup of 1024: per cloud index w, the exclusive scan of total[b][w] over the pairs -> offsets [B + 1][2]
__global__ __launch_bounds__(1024) void tracklet_scan_kernel(const int* __restrict__ total, long long* __restrict__ offsets, int B)
{
  __shared__ long long part[1024];
  const int tid = threadIdx.x;
  const long long n = B, per = (n + 1023) / 1024;
  for (int w = 0; w < 2; ++w) {
    const long long lo = min(n, tid * per), hi = min(n, lo + per);
    long long s = 0;
    for (long long b = lo; b < hi; ++b) s += total[b * 2 + w];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
      long long run = 0;
      for (int i = 0; i < 1024; ++i) { const long long v = part[i]; part[i] = run; run += v; }
      offsets[n * 2 + w] = run;
    }
    __syncthreads();
    long long run = part[tid];
    for (long long b = lo; b < hi; ++b) { offsets[b * 2 + w] = run; run += total[b * 2 + w]; }
    __syncthreads();
  }
}

// grid: the (frame, chunk) items
template <class C, int STRIDE>
__global__ __launch_bounds__(kThreads) void crop_scatter_kernel(const float* __restrict__ scans, const CropFrame* __restrict__ frames,
                                                                const int2* __restrict__ items, const typename C::Job* __restrict__ jobs,
                                                                const typename C::Cal* __restrict__ cals, const int* __restrict__ counts,
                                                                const int* __restrict__ pos, const long long* __restrict__ offsets,
                                                                float* __restrict__ out0, float* __restrict__ out1)
{
  __shared__ int wcnt[kQuarters][4];
  const int2 it = items[blockIdx.x];
  const CropFrame f = frames[it.x];
  const int chunk = it.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  Pt p[kQuarters]; typename C::Prep q[kQuarters];
  bool loaded = false;
  for (int j0 = 0; j0 < f.njobs; j0 += 64) {
    // the counts of 64 jobs at once, a lane each: every wave reads the same numbers, so `hit` is the same in the whole workgroup
    const int mine_job = j0 + lane;
    const int cnt = mine_job < f.njobs ? counts[jobs[f.job0 + mine_job].cbase + chunk] : 0;
    unsigned long long hit = __ballot(cnt != 0);
    while (hit) {
      const int jj = j0 + __ffsll((long long)hit) - 1;
      hit &= hit - 1;
      if (!loaded) {
        bool valid[kQuarters];
        load_points<STRIDE>(scans, f, chunk, p, valid);
        C::prepare(cals, f, p, valid, q);
        loaded = true;
      }
      const typename C::Job j = jobs[f.job0 + jj];
      unsigned long long m[kQuarters];
#pragma unroll
      for (int i = 0; i < kQuarters; ++i) {
        m[i] = C::ballot(j, p[i], q[i]);
        if (lane == 0) wcnt[i][wave] = __popcll(m[i]);
      }
      __syncthreads();
      float* out = (j.which ? out1 : out0) + (offsets[(long long)j.pair * 2 + j.which] + pos[j.cbase + chunk]) * 3;
      int before = 0;   // members of this (job, chunk) ahead of the wave's 64 points of quarter i: scan order is (quarter, wave, lane)
#pragma unroll
      for (int i = 0; i < kQuarters; ++i) {
        int mine = before;
#pragma unroll
        for (int w = 0; w < 4; ++w) { const int n = wcnt[i][w]; if (w < wave) mine += n; before += n; }
        if ((m[i] >> lane) & 1ull) {
          float* o = out + (size_t)(mine + __popcll(m[i] & ((1ull << lane) - 1ull))) * 3;
          o[0] = p[i].x; o[1] = p[i].y; o[2] = p[i].z - j.dz;
        }
      }
      __syncthreads();
    }
  }
}

// ---- the image-frustum crop ------------------------------------------------------------------------------------------------------------------
struct FrustumJob {
  double xmin, ymin, xmax, ymax;   // the 2D box, pixels
  long long cbase;                 // as CropJob's
  float dz;
  int which, pair, pad;
};
static_assert(sizeof(FrustumJob) == 56, "LDS budget");

struct FrustumCal { double m[12], W, H, clip; };   // of an uploaded frame: M row-major, the image size, the clip distance

struct Px { double u, v; bool ok; };   // a projected point; ok: finite, in front of the clip distance and in the image

__device__ __forceinline__ Px frustum_project(const FrustumCal& c, const Pt& p, bool valid)
{
#pragma clang fp contract(off)
  const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
  const double w0 = ((c.m[0] * x + c.m[1] * y) + c.m[2] * z) + c.m[3];
  const double w1 = ((c.m[4] * x + c.m[5] * y) + c.m[6] * z) + c.m[7];
  const double w2 = ((c.m[8] * x + c.m[9] * y) + c.m[10] * z) + c.m[11];
  Px q;
  q.u = w0 / w2; q.v = w1 / w2;
  // a NaN or infinite u / v fails a comparison of every pair below
  q.ok = valid && isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && x > c.clip && 0.0 <= q.u && q.u < c.W && 0.0 <= q.v && q.v < c.H;
  return q;
}

__device__ __forceinline__ bool frustum_inside(const FrustumJob& j, const Px& q)
{
  return q.ok && j.xmin <= q.u && q.u < j.xmax && j.ymin <= q.v && q.v < j.ymax;
}

struct FrustumCrop {
  typedef FrustumJob Job;
  typedef FrustumCal Cal;
  typedef Px Prep;
  // the calibration belongs to the frame: a point is projected once per chunk, not per job
  static __device__ __forceinline__ void prepare(const Cal* __restrict__ cals, const CropFrame& f, const Pt* p, const bool* valid, Prep* q)
  {
    const FrustumCal cal = cals[f.frame];
#pragma unroll
    for (int i = 0; i < kQuarters; ++i) q[i] = frustum_project(cal, p[i], valid[i]);
  }
  static __device__ __forceinline__ unsigned long long ballot(const Job& j, const Pt&, const Prep& q) { return __ballot(frustum_inside(j, q)); }
};

// ---- host state ------------------------------------------------------------------------------------------------------------------------------
struct TrackletWS {
  // uploaded scans (alignnet_tracklet_upload_scans)
  int F = -1, stride = 0;                   // F = -1: nothing uploaded
  std::vector<long long> foff;              // [F + 1] first point of every frame
  float* d_scans = nullptr;
  // work buffers, grown on demand
  char* d_jobs = nullptr; size_t cap_jobs = 0;   // the call's C::Job table, in bytes
  FrustumCal* d_cals = nullptr; size_t cap_cals = 0;
  CropFrame* d_frames = nullptr; size_t cap_frames = 0;
  int2* d_items = nullptr; size_t cap_items = 0;
  int* d_counts = nullptr; int* d_pos = nullptr; size_t cap_counts = 0, cap_pos = 0;
  JobSpan* d_spans = nullptr; int* d_total = nullptr; size_t cap_spans = 0, cap_total = 0;
  long long* d_offsets = nullptr; size_t cap_off = 0;
  // the last result (alignnet_tracklet_extract) and the blobs the next one is built in
  int B = -1;
  std::vector<long long> offsets;           // [B + 1][2]
  float* d_pts[2] = {nullptr, nullptr}; size_t cap_pts[2] = {0, 0};
  float* d_next[2] = {nullptr, nullptr}; size_t cap_next[2] = {0, 0};
};

TrackletWS* tws(alignnet_handle* h) { return static_cast<TrackletWS*>(h->tracklet_ws); }

// the float32 bound of the pre-test: (r + |b| 6e-8)(1 + 1e-6) rounded up (the header of this file); not finite -> nothing is rejected
float pre_bound(double r, double b)
{
  const double t = (r + std::fabs(b) * 6e-8) * (1.0 + 1e-6);
  if (!(t < 3e38)) return INFINITY;
  return std::nextafter((float)t, INFINITY);
}

std::string job_where(int j) { return " (pair " + std::to_string(j / 2) + ", cloud " + std::to_string(j % 2 + 1) + ")"; }

// the two kernels of policy C over the (frame, chunk) items, for the stride of the uploaded scans
template <class C>
void launch_test(alignnet_handle* h, const TrackletWS* w, unsigned items, const typename C::Job* jobs, const typename C::Cal* cals)
{
  if (w->stride == 4)
    hipLaunchKernelGGL((crop_test_kernel<C, 4>), dim3(items), dim3(kThreads), 0, h->stream, w->d_scans, w->d_frames, w->d_items, jobs, cals, w->d_counts);
  else
    hipLaunchKernelGGL((crop_test_kernel<C, 3>), dim3(items), dim3(kThreads), 0, h->stream, w->d_scans, w->d_frames, w->d_items, jobs, cals, w->d_counts);
}

template <class C>
void launch_scatter(alignnet_handle* h, const TrackletWS* w, unsigned items, const typename C::Job* jobs, const typename C::Cal* cals)
{
  if (w->stride == 4)
    hipLaunchKernelGGL((crop_scatter_kernel<C, 4>), dim3(items), dim3(kThreads), 0, h->stream, w->d_scans, w->d_frames, w->d_items, jobs, cals, w->d_counts,
                       w->d_pos, w->d_offsets, w->d_next[0], w->d_next[1]);
  else
    hipLaunchKernelGGL((crop_scatter_kernel<C, 3>), dim3(items), dim3(kThreads), 0, h->stream, w->d_scans, w->d_frames, w->d_items, jobs, cals, w->d_counts,
                       w->d_pos, w->d_offsets, w->d_next[0], w->d_next[1]);
}

// What the box (C = BoxCrop) and the frustum (FrustumCrop) extraction share: the checks of the call and of every job's frame and dz, the tables
// (entries of the counts table in (pair, cloud, chunk) order; jobs sorted by frame), the three stages and the swap of the result blobs.
// check(F) and check_job(j) are the entry point's checks of its own arguments, of the call against the F uploaded frames and of job j = 2 pair +
// cloud (they return fail()'s 1), called where the entry points made them before the checks were shared; the frustum's check(F) fills `cals`,
// the calibration of every uploaded frame, which stays empty for the box.  fill(job, j) sets what the test of job j needs.
template <class C, typename Check, typename CheckJob, typename Fill>
int run_extract(alignnet_handle* h, const std::string& name, const int32_t* frames, const float* dz, int32_t B, const std::vector<FrustumCal>& cals,
                Check check, CheckJob check_job, Fill fill, int64_t* offsets)
{
  typedef typename C::Job Job;
  if (!h->tracklet_ws || tws(h)->F < 0) return fail(h, name + ": no scans uploaded");
  if (B < 0 || B > (1 << 24)) return fail(h, name + ": B out of range");
  TrackletWS* w = tws(h);
  const int J = 2 * B;
  if (check(w->F)) return 1;
  for (int j = 0; j < J; ++j) {
    if (frames[j] < 0 || frames[j] >= w->F) return fail(h, name + ": frame " + std::to_string(frames[j]) + " out of range" + job_where(j));
    if (check_job(j)) return 1;
    if (!std::isfinite(dz[j])) return fail(h, name + ": non-finite dz" + job_where(j));
  }
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  std::vector<JobSpan> spans(J);
  long long entries_ll = 0;
  for (int j = 0; j < J; ++j) {
    const long long ch = (w->foff[frames[j] + 1] - w->foff[frames[j]] + kChunk - 1) / kChunk;
    spans[j].cbase = entries_ll; spans[j].chunks = (int)ch; spans[j].pad = 0;
    entries_ll += ch;
  }
  const size_t entries = (size_t)entries_ll;
  std::vector<int> order(J);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return frames[a] < frames[b]; });
  std::vector<Job> jobs(J);
  std::vector<CropFrame> groups;
  std::vector<int2> items;
  for (int i = 0; i < J; ++i) {
    const int j = order[i];
    Job& c = jobs[i];
    fill(c, j);
    c.dz = dz[j]; c.cbase = spans[j].cbase; c.which = j % 2; c.pair = j / 2;
    if (groups.empty() || frames[j] != frames[order[i - 1]]) {
      CropFrame g;
      g.pt0 = w->foff[frames[j]]; g.n = (int)(w->foff[frames[j] + 1] - w->foff[frames[j]]); g.job0 = i; g.njobs = 0; g.frame = frames[j];
      for (int ch = 0; ch < (g.n + kChunk - 1) / kChunk; ++ch) items.push_back(make_int2((int)groups.size(), ch));
      groups.push_back(g);
    }
    ++groups.back().njobs;
  }
  if (items.size() > 0x7fffffffull) return fail(h, name + ": too many (frame, chunk) work items");
  std::vector<long long> off((size_t)(B + 1) * 2, 0);
  if (J > 0) {
    if ((!cals.empty() && grow(h, &w->d_cals, &w->cap_cals, cals.size())) || grow(h, &w->d_jobs, &w->cap_jobs, jobs.size() * sizeof(Job)) ||
        grow(h, &w->d_frames, &w->cap_frames, groups.size()) || grow(h, &w->d_items, &w->cap_items, items.size()) ||
        grow(h, &w->d_counts, &w->cap_counts, entries) || grow(h, &w->d_pos, &w->cap_pos, entries) ||
        grow(h, &w->d_spans, &w->cap_spans, spans.size()) || grow(h, &w->d_total, &w->cap_total, spans.size()) ||
        grow(h, &w->d_offsets, &w->cap_off, off.size()))
      return 1;
    const typename C::Cal* d_cals = cals.empty() ? nullptr : w->d_cals;
    const Job* d_jobs = reinterpret_cast<const Job*>(w->d_jobs);   // an allocation's base: aligned for either kind
    HIP_TRY(h, hipMemcpyAsync(w->d_jobs, jobs.data(), jobs.size() * sizeof(Job), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(w->d_frames, groups.data(), groups.size() * sizeof(CropFrame), hipMemcpyHostToDevice, h->stream));
    if (!items.empty()) HIP_TRY(h, hipMemcpyAsync(w->d_items, items.data(), items.size() * sizeof(int2), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(w->d_spans, spans.data(), spans.size() * sizeof(JobSpan), hipMemcpyHostToDevice, h->stream));
    if (!items.empty()) {
      alignnet::ProfScope prof_scope(h, alignnet::PK_TRACKLET_TEST);
      // with the other tables: the stream is synchronised before the caller's `cals` goes (an error of the copy is the next hipGetLastError's)
      if (d_cals) (void)hipMemcpyAsync(w->d_cals, cals.data(), cals.size() * sizeof(FrustumCal), hipMemcpyHostToDevice, h->stream);
      launch_test<C>(h, w, (unsigned)items.size(), d_jobs, d_cals);
    }
    {
      alignnet::ProfScope prof_scope(h, alignnet::PK_TRACKLET_COMPACT);
      hipLaunchKernelGGL(tracklet_jobscan_kernel, dim3((unsigned)J), dim3(kThreads), 0, h->stream, w->d_counts, w->d_spans, w->d_pos, w->d_total);
      hipLaunchKernelGGL(tracklet_scan_kernel, dim3(1), dim3(1024), 0, h->stream, w->d_total, w->d_offsets, B);
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(off.data(), w->d_offsets, off.size() * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int k = 0; k < 2; ++k)
      if (grow(h, &w->d_next[k], &w->cap_next[k], (size_t)off[(size_t)B * 2 + k] * 3)) return 1;
    if (!items.empty() && off[(size_t)B * 2] + off[(size_t)B * 2 + 1] > 0) {
      alignnet::ProfScope prof_scope(h, alignnet::PK_TRACKLET_COMPACT);
      launch_scatter<C>(h, w, (unsigned)items.size(), d_jobs, d_cals);
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int k = 0; k < 2; ++k) { std::swap(w->d_pts[k], w->d_next[k]); std::swap(w->cap_pts[k], w->cap_next[k]); }
  }
  w->offsets.swap(off);
  w->B = B;
  if (offsets) for (size_t i = 0; i < w->offsets.size(); ++i) offsets[i] = w->offsets[i];
  return 0;
}

}  // namespace

extern "C" int alignnet_tracklet_free_scans(alignnet_handle* h)
{
  if (!h) return 1;
  if (!h->tracklet_ws) return 0;
  TrackletWS* w = tws(h);
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (w->d_scans) hipFree(w->d_scans);
  w->d_scans = nullptr; w->F = -1; w->stride = 0; w->foff.clear();
  return 0;
}

extern "C" void alignnet_tracklet_free(alignnet_handle* h)
{
  if (!h || !h->tracklet_ws) return;
  TrackletWS* w = tws(h);
  if (h->stream) hipStreamSynchronize(h->stream);
  void* const ptrs[] = {w->d_scans, w->d_jobs, w->d_cals, w->d_frames, w->d_items, w->d_counts, w->d_pos, w->d_spans, w->d_total, w->d_offsets,
                        w->d_pts[0], w->d_pts[1], w->d_next[0], w->d_next[1]};
  for (void* p : ptrs) if (p) hipFree(p);
  delete w;
  h->tracklet_ws = nullptr;
}

extern "C" int alignnet_tracklet_upload_scans(alignnet_handle* h, const float* points, int32_t stride, const int64_t* offsets, int32_t F)
{
  if (!h) return 1;
  const std::string name("alignnet_tracklet_upload_scans");
  if (stride != 3 && stride != 4) return fail(h, name + ": stride must be 3 or 4 floats per point");
  if (F < 0 || !offsets) return fail(h, name + ": F < 0 or null offsets");
  if (offsets[0] != 0) return fail(h, name + ": offsets must start at 0");
  for (int f = 0; f < F; ++f) {
    if (offsets[f + 1] < offsets[f]) return fail(h, name + ": offsets must be non-decreasing");
    if (offsets[f + 1] - offsets[f] > 0x7fffffff - kChunk) return fail(h, name + ": frame " + std::to_string(f) + " too large");
  }
  const size_t n = (size_t)offsets[F];
  if (n && !points) return fail(h, name + ": null points");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  float* d = nullptr;
  HIP_TRY(h, hipMalloc(&d, std::max<size_t>(n, 1) * stride * sizeof(float)));
  if (n) {
    const hipError_t e = hipMemcpy(d, points, n * stride * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { hipFree(d); return fail(h, name + ": hipMemcpy: " + hipGetErrorString(e)); }
  }
  if (!h->tracklet_ws) h->tracklet_ws = new TrackletWS();
  if (alignnet_tracklet_free_scans(h)) { hipFree(d); return 1; }
  TrackletWS* w = tws(h);
  w->d_scans = d; w->F = F; w->stride = stride;
  w->foff.assign(offsets, offsets + (size_t)F + 1);
  return 0;
}

extern "C" int alignnet_tracklet_extract(alignnet_handle* h, const int32_t* frames, const double* boxes, const float* dz, int32_t B, int64_t* offsets)
{
  if (!h) return 1;
  const std::string name("alignnet_tracklet_extract");
  return run_extract<BoxCrop>(
      h, name, frames, dz, B, std::vector<FrustumCal>(),
      [&](int) { return B > 0 && (!frames || !boxes || !dz) ? fail(h, name + ": null argument") : 0; },
      [&](int j) {
        for (int k = 0; k < 7; ++k) if (!std::isfinite(boxes[(size_t)j * 7 + k])) return fail(h, name + ": non-finite box value" + job_where(j));
        for (int k = 3; k < 6; ++k) if (boxes[(size_t)j * 7 + k] < 0.0) return fail(h, name + ": negative box extent" + job_where(j));
        return 0;
      },
      [&](CropJob& c, int j) {
        const double* b = boxes + (size_t)j * 7;
        c.bx = b[0]; c.by = b[1]; c.bz = b[2];
        c.c = std::cos(b[6]); c.s = std::sin(b[6]);
        c.h = b[3]; c.hw = b[4] * 0.5; c.hl = b[5] * 0.5;
        const double rxz = std::hypot(c.hl, c.hw) * (1.0 + 1e-12);
        c.fx = (float)b[0]; c.fy = (float)b[1]; c.fz = (float)b[2];
        c.txz = pre_bound(rxz, std::max(std::fabs(b[0]), std::fabs(b[2])));
        c.ty = pre_bound(c.h, b[1]);
      },
      offsets);
}

extern "C" int alignnet_tracklet_extract_frustum(alignnet_handle* h, const int32_t* frames, const double* rects, const float* dz, int32_t B,
                                                 const double* proj, const double* image, double clip, int64_t* offsets)
{
  if (!h) return 1;
  const std::string name("alignnet_tracklet_extract_frustum");
  std::vector<FrustumCal> cals;   // lives until run_extract has synchronised the stream
  return run_extract<FrustumCrop>(
      h, name, frames, dz, B, cals,
      [&](int F) {
        if ((B > 0 && (!frames || !rects || !dz)) || (F > 0 && (!proj || !image))) return fail(h, name + ": null argument");
        if (!std::isfinite(clip)) return fail(h, name + ": non-finite clip");
        for (int f = 0; f < F; ++f) {
          const std::string where = " (frame " + std::to_string(f) + ")";
          for (int k = 0; k < 12; ++k) if (!std::isfinite(proj[(size_t)f * 12 + k])) return fail(h, name + ": non-finite proj value" + where);
          for (int k = 0; k < 2; ++k) {
            if (!std::isfinite(image[(size_t)f * 2 + k])) return fail(h, name + ": non-finite image size" + where);
            if (image[(size_t)f * 2 + k] <= 0.0) return fail(h, name + ": image size <= 0" + where);
          }
        }
        if (B > 0) {
          // the calibration of every uploaded frame (120 bytes each), indexed by CropFrame::frame
          cals.resize(F);
          for (int f = 0; f < F; ++f) {
            std::copy(proj + (size_t)f * 12, proj + (size_t)f * 12 + 12, cals[f].m);
            cals[f].W = image[(size_t)f * 2]; cals[f].H = image[(size_t)f * 2 + 1]; cals[f].clip = clip;
          }
        }
        return 0;
      },
      [&](int j) {
        for (int k = 0; k < 4; ++k) if (!std::isfinite(rects[(size_t)j * 4 + k])) return fail(h, name + ": non-finite rect value" + job_where(j));
        return 0;
      },
      [&](FrustumJob& c, int j) {
        const double* r = rects + (size_t)j * 4;
        c.xmin = r[0]; c.ymin = r[1]; c.xmax = r[2]; c.ymax = r[3]; c.pad = 0;
      },
      offsets);
}

extern "C" int alignnet_tracklet_read(alignnet_handle* h, float* points1, float* points2)
{
  if (!h) return 1;
  if (!h->tracklet_ws || tws(h)->B < 0) return fail(h, "alignnet_tracklet_read: nothing extracted yet");
  TrackletWS* w = tws(h);
  float* const dst[2] = {points1, points2};
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  for (int k = 0; k < 2; ++k) {
    const size_t n = (size_t)w->offsets[(size_t)w->B * 2 + k];
    if (n && dst[k]) HIP_TRY(h, hipMemcpyAsync(dst[k], w->d_pts[k], n * 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int alignnet_tracklet_install_dataset(alignnet_handle* h, const float* labels)
{
  if (!h) return 1;
  if (!h->tracklet_ws || tws(h)->B < 0) return fail(h, "alignnet_tracklet_install_dataset: nothing extracted yet");
  TrackletWS* w = tws(h);
  if (w->B < 1 || !labels) return fail(h, "alignnet_tracklet_install_dataset: no pairs or null labels");
  static_assert(sizeof(long long) == sizeof(int64_t), "offsets");
  return alignnet_dataset_install(h, w->d_pts[0], w->d_pts[1], true, reinterpret_cast<const int64_t*>(w->offsets.data()), labels, w->B,
                                  "alignnet_tracklet_install_dataset");
}
