// Multi-scale (coarse-to-fine) ICP (include/alignnet_hip.h: alignnet_icp_multiscale_register*), gfx950 only.  Definition: tests/icp_multiscale_ref.py.
//
// Both clouds of every pair are voxel-downsampled at the voxel sizes of the call's levels (tests/global_reg_ref.py::voxel_downsample, the mean rounded
// to float32), and the ICP of alignnet_icp_register / _plane_register / _generalized_register runs level by level, each level from the transform the
// level before left on the device (alignnet_icp_run_device).  A level with voxel <= 0 runs on the raw clouds and tables: nothing is copied.
//
// The pyramid is three launches over all (cloud, downsampled level), cloud c = 2 * pair + side:
//   ms_sort_kernel   one workgroup per (cloud, level): the float32 minimum, the 63-bit voxel keys in fp64, a bitonic sort of (key, point index) and
//                    the number of distinct keys.  The network is the all-ascending form (a mirror step, then half-cleaners), so positions past the
//                    cloud's n stand for +inf without being stored: any n sorts in n records, no power-of-two padding in HBM.  A cloud of at most
//                    kMsChunk points sorts in LDS; a larger one sorts chunks of kMsChunk in LDS and runs only the steps that span chunks (j >=
//                    kMsChunk) through HBM, each followed by one LDS pass per chunk: 10 passes over a 58,600-point cloud instead of 136.
//   ms_scan_kernel   one wave per (side, level): the exclusive scan of the counts over the pairs = that level's offsets table [B + 1][2], so the
//                    level's clouds lie back to back exactly as the ICP kernels address a call's clouds.
//   ms_emit_kernel   one workgroup per (cloud, level): every thread takes a contiguous range of the sorted records and, for every voxel that begins
//                    in it, sums the voxel's points in fp64 in ascending point index (the sort's second key), divides by the count and stores the
//                    float32 point at the voxel's rank.  No floating-point atomics anywhere; the only atomic is the integer error flag.
// Every loop is bounded by the cloud's size; nothing waits for another workgroup.  What a (cloud, level) produces depends on the cloud's points and
// the voxel size alone.
#include "engine.h"
#include "host_util.h"
#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr int kMsThreads = 1024, kMsWaves = kMsThreads / 64;
constexpr int kMsChunk = 8192;                 // (key, index) records sorted in LDS at once: 12 bytes each
constexpr int kMsScratch = 256;                // bytes of reduction scratch behind the records
constexpr int kMsMaxLevels = 8;
constexpr long long kMsMaxPoints = 1ll << 30;  // of one cloud (the network's power of two stays an int)
constexpr unsigned long long kMsInf = ~0ull;   // a key no point has (the real ones hold 63 bits)

struct MsArgs {
  const float* pts[2]; const long long* off; const int* rows;   // the raw clouds as the ICP kernels address them
  int B, Ld;                        // pairs; downsampled levels
  double voxel[kMsMaxLevels];       // their voxel edges
  const long long* slot;            // [2 B] where cloud c's sort records start; every level has slot_total of them
  long long slot_total;
  unsigned long long* key; int* val;
  long long* cnt;                   // [Ld][B][2] voxels of (level, pair, side)
  long long* lvl_off;               // [Ld][B + 1][2] the levels' offsets tables
  float* lvl_pts[2];                // [Ld][total[side]][3] the levels' clouds
  long long total[2];               // raw points per side
  int* err;
  double* dbg_mean; int* dbg_vox; int* dbg_cnt;   // alignnet_debug_voxel_pyramid: records of side 0, laid out as lvl_pts[0]; null otherwise
};

__device__ __forceinline__ void ms_cloud(const MsArgs& a, int c, const float** p, long long* n)
{
  const int b = c >> 1, side = c & 1;
  const long long row = a.rows ? a.rows[b] : b;
  const long long lo = a.off[row * 2 + side];
  *n = a.off[(row + 1) * 2 + side] - lo;
  *p = a.pts[side] + lo * 3;
}

// ascending compare-exchange of records i < l by (key, point index)
template <class K, class V>
__device__ __forceinline__ void ms_cx(K* key, V* val, int i, int l)
{
  const unsigned long long ki = key[i], kl = key[l];
  const int vi = val[i], vl = val[l];
  if (ki > kl || (ki == kl && vi > vl)) { key[i] = kl; key[l] = ki; val[i] = vl; val[l] = vi; }
}

// comparator q of a step: the mirror step of blocks of k (i in the lower half against its mirror image) or the half-cleaner at distance j
__device__ __forceinline__ void ms_pair_mirror(int q, int k, int* i, int* l)
{
  const int half = k >> 1;
  *i = ((q & ~(half - 1)) << 1) | (q & (half - 1));
  *l = *i ^ (k - 1);
}
__device__ __forceinline__ void ms_pair_clean(int q, int j, int* i, int* l)
{
  *i = ((q & ~(j - 1)) << 1) | (q & (j - 1));
  *l = *i | j;
}

// the half-cleaners j = jtop, jtop / 2, .. 1 on C records in LDS
__device__ __forceinline__ void ms_lds_clean(unsigned long long* lk, int* lv, int C, int jtop)
{
  for (int j = jtop; j > 0; j >>= 1) {
    for (int q = threadIdx.x; q < (C >> 1); q += kMsThreads) { int i, l; ms_pair_clean(q, j, &i, &l); ms_cx(lk, lv, i, l); }
    __syncthreads();
  }
}

// every step k = 2 .. C on C records in LDS
__device__ __forceinline__ void ms_lds_sort(unsigned long long* lk, int* lv, int C)
{
  for (int k = 2; k <= C; k <<= 1) {
    for (int q = threadIdx.x; q < (C >> 1); q += kMsThreads) { int i, l; ms_pair_mirror(q, k, &i, &l); ms_cx(lk, lv, i, l); }
    __syncthreads();
    ms_lds_clean(lk, lv, C, k >> 2);
  }
}

__global__ __launch_bounds__(kMsThreads) void ms_sort_kernel(const MsArgs a)
{
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char ms_lds[];
  const int c = blockIdx.x, ld = blockIdx.y, tid = threadIdx.x;
  const float* p; long long nl;
  ms_cloud(a, c, &p, &nl);
  const int n = (int)nl;
  long long* const cnt = a.cnt + ((size_t)ld * a.B + (c >> 1)) * 2 + (c & 1);
  if (n == 0) { if (tid == 0) *cnt = 0; return; }
  int P = 1;
  while (P < n) P <<= 1;
  const int C = min(P, kMsChunk);
  unsigned long long* lk = reinterpret_cast<unsigned long long*>(ms_lds);
  int* lv = reinterpret_cast<int*>(ms_lds + (size_t)C * 8);
  float* smin = reinterpret_cast<float*>(ms_lds + (size_t)C * 12);          // [3][kMsWaves]
  int* sh = reinterpret_cast<int*>(ms_lds + (size_t)C * 12 + 3 * kMsWaves * 4);   // [kMsWaves]
  unsigned long long* gk = a.key + (size_t)ld * a.slot_total + a.slot[c];
  int* gv = a.val + (size_t)ld * a.slot_total + a.slot[c];
  const double v = a.voxel[ld];

  // origin: the float32 minimum per axis, widened, minus half an edge
  float mn[3] = {INFINITY, INFINITY, INFINITY};
  for (int i = tid; i < n; i += kMsThreads)
#pragma unroll
    for (int k = 0; k < 3; ++k) mn[k] = fminf(mn[k], p[(size_t)i * 3 + k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn[k] = fminf(mn[k], __shfl_xor(mn[k], o));
    if ((tid & 63) == 0) smin[k * kMsWaves + (tid >> 6)] = mn[k];
  }
  __syncthreads();
  double m0[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float w = smin[k * kMsWaves];
    for (int i = 1; i < kMsWaves; ++i) w = fminf(w, smin[k * kMsWaves + i]);
    m0[k] = (double)w - v / 2.0;
  }

  int heads = 0;   // distinct keys this thread met while it stored final records
  // the records of chunk [base, base + C) go back to HBM; with `last` they are final and the distinct keys are counted
  auto store = [&](int base, bool last) {
    for (int t = tid; t < C && base + t < n; t += kMsThreads) {
      const unsigned long long k = lk[t];
      gk[base + t] = k; gv[base + t] = lv[t];
      if (last) heads += (base + t == 0 || k != (t ? lk[t - 1] : gk[base - 1])) ? 1 : 0;   // (the chunk before is final and stored: the barrier below)
    }
    __syncthreads();
  };

  // every chunk: keys from the points, sorted in LDS
  for (int base = 0; base < n; base += C) {
    for (int t = tid; t < C; t += kMsThreads) {
      const int i = base + t;
      unsigned long long kk = kMsInf;
      if (i < n) {
        kk = 0;
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double f = floor(((double)p[(size_t)i * 3 + k] - m0[k]) / v);
          if (f >= 0.0 && f < 2097152.0) kk = (kk << 21) | (unsigned long long)(long long)f; else ok = false;
        }
        if (!ok) { kk = 0; atomicOr(a.err, 1); }   // not finite, or wider than 2^21 voxels: the host reports it, nothing is truncated
      }
      lk[t] = kk; lv[t] = i < n ? i : 0x7fffffff;
    }
    __syncthreads();
    ms_lds_sort(lk, lv, C);
    store(base, P == C);
  }
  // the steps that span chunks: their wide comparators through HBM (a partner at or past n is +inf: no exchange), the rest per chunk in LDS
  for (int k = C << 1; k <= P && k > 0; k <<= 1) {
    for (int j = k >> 1; j >= C; j >>= 1) {
      const bool mirror = j == (k >> 1);
      for (int q = tid; q < (P >> 1); q += kMsThreads) {
        int i, l;
        if (mirror) ms_pair_mirror(q, k, &i, &l); else ms_pair_clean(q, j, &i, &l);
        if (l < n) ms_cx(gk, gv, i, l);
      }
      __syncthreads();
    }
    for (int base = 0; base < n; base += C) {
      for (int t = tid; t < C; t += kMsThreads) {
        const int i = base + t;
        lk[t] = i < n ? gk[i] : kMsInf; lv[t] = i < n ? gv[i] : 0x7fffffff;
      }
      __syncthreads();
      ms_lds_clean(lk, lv, C, C >> 1);
      store(base, k == P);
    }
  }
  // the cloud's voxels
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) heads += __shfl_xor(heads, o);
  if ((tid & 63) == 0) sh[tid >> 6] = heads;
  __syncthreads();
  if (tid == 0) { int m = 0; for (int i = 0; i < kMsWaves; ++i) m += sh[i]; *cnt = m; }
}

// one wave per (side, level): lvl_off[.][b][side] = the voxels of pairs before b, [B] = all
__global__ __launch_bounds__(64) void ms_scan_kernel(const MsArgs a)
{
  const int side = blockIdx.x, ld = blockIdx.y, lane = threadIdx.x;
  const long long* cnt = a.cnt + (size_t)ld * a.B * 2 + side;
  long long* off = a.lvl_off + (size_t)ld * (a.B + 1) * 2 + side;
  long long carry = 0;
  for (int b0 = 0; b0 < a.B; b0 += 64) {
    const int b = b0 + lane;
    const long long x = b < a.B ? cnt[(size_t)b * 2] : 0;
    long long inc = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const long long t = __shfl_up(inc, o); if (lane >= o) inc += t; }
    if (b < a.B) off[(size_t)b * 2] = carry + inc - x;
    carry += __shfl(inc, 63);
  }
  if (lane == 0) off[(size_t)a.B * 2] = carry;
}

__global__ __launch_bounds__(kMsThreads) void ms_emit_kernel(const MsArgs a)
{
#pragma clang fp contract(off)
  __shared__ int sh[kMsWaves + 1];
  const int c = blockIdx.x, ld = blockIdx.y, tid = threadIdx.x, side = c & 1;
  const float* p; long long nl;
  ms_cloud(a, c, &p, &nl);
  const int n = (int)nl;
  if (n == 0) return;
  const unsigned long long* gk = a.key + (size_t)ld * a.slot_total + a.slot[c];
  const int* gv = a.val + (size_t)ld * a.slot_total + a.slot[c];
  const size_t at = (size_t)ld * a.total[side] + a.lvl_off[((size_t)ld * (a.B + 1) + (c >> 1)) * 2 + side];   // the cloud's first point in the level's blob
  float* out = a.lvl_pts[side] + at * 3;
  const bool dbg = a.dbg_mean && side == 0;
  // this thread's records, and the rank of the first voxel that begins among them
  const int per = (n + kMsThreads - 1) / kMsThreads;
  const int s0 = min(n, tid * per), s1 = min(n, s0 + per);
  int heads = 0;
  for (int i = s0; i < s1; ++i) heads += (i == 0 || gk[i] != gk[i - 1]) ? 1 : 0;
  const int lane = tid & 63, w = tid >> 6;
  int inc = heads;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  if (tid == 0) { int s = 0; for (int i = 0; i < kMsWaves; ++i) { const int t = sh[i]; sh[i] = s; s += t; } }
  __syncthreads();
  int o = sh[w] + inc - heads;
  for (int i = s0; i < s1; ++i) {
    const unsigned long long kk = gk[i];
    if (i != 0 && kk == gk[i - 1]) continue;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int e = i;
    for (; e < n && gk[e] == kk; ++e) {   // ascending point index (a voxel may run on into the next thread's records)
      const size_t s = (size_t)gv[e] * 3;
      sx += (double)p[s]; sy += (double)p[s + 1]; sz += (double)p[s + 2];
    }
    const double num = (double)(e - i);
    const double mx = sx / num, my = sy / num, mz = sz / num;
    out[(size_t)o * 3] = (float)mx; out[(size_t)o * 3 + 1] = (float)my; out[(size_t)o * 3 + 2] = (float)mz;
    if (dbg) {
      const size_t r = at + o;
      a.dbg_mean[r * 3] = mx; a.dbg_mean[r * 3 + 1] = my; a.dbg_mean[r * 3 + 2] = mz;
      a.dbg_vox[r * 3] = (int)(kk >> 42); a.dbg_vox[r * 3 + 1] = (int)((kk >> 21) & 0x1fffff); a.dbg_vox[r * 3 + 2] = (int)(kk & 0x1fffff);
      a.dbg_cnt[r] = e - i;
    }
    ++o;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------
size_t ms_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// a call's carve of the handle's workspace
struct MsCarve {
  size_t bytes = 0;
  size_t take(size_t b) { const size_t at = bytes; bytes += ms_align(b); return at; }
};

// if a call leaves early, the copies it queued from its own host vectors must have run before those go away
struct MsDrain {
  hipStream_t s; bool armed = true;
  ~MsDrain() { if (armed) hipStreamSynchronize(s); }
};

struct MsSchedule { int L; const double* voxel; const double* radius; const int32_t* its; const double* normal_radius; int estimate; bool full; };

int ms_schedule(alignnet_handle* h, const std::string& fn, int32_t L, const double* voxel_sizes, const double* radii, const int32_t* its,
                const double* normal_radii, int32_t estimate, int32_t flags, MsSchedule* s)
{
  if (flags & ~1) return fail(h, fn + ": unknown flags " + std::to_string(flags) + " (bit 0 = full rotation is the only one)");
  if (L < 1 || L > kMsMaxLevels) return fail(h, fn + ": L must be in [1, " + std::to_string(kMsMaxLevels) + "], got " + std::to_string(L));
  if (!voxel_sizes || !radii || !its) return fail(h, fn + ": null voxel_sizes / radii / its");
  if (estimate != 1 && estimate != 2 && estimate != 4)
    return fail(h, fn + ": estimate must be 1 (point-to-point), 2 (point-to-plane) or 4 (generalized), got " + std::to_string(estimate));
  if (estimate >= 2 && !normal_radii) return fail(h, fn + ": null normal_radii (the plane and generalized estimates need one per level)");
  for (int l = 0; l < L; ++l) {
    if (!std::isfinite(voxel_sizes[l])) return fail(h, fn + ": voxel_sizes[" + std::to_string(l) + "] is not finite");
    if (!(radii[l] > 0.0)) return fail(h, fn + ": radii[" + std::to_string(l) + "] must be > 0");
    if (its[l] < 0) return fail(h, fn + ": its[" + std::to_string(l) + "] must be >= 0");
    if (estimate >= 2 && !(normal_radii[l] > 0.0)) return fail(h, fn + ": normal_radii[" + std::to_string(l) + "] must be > 0");
  }
  *s = MsSchedule{L, voxel_sizes, radii, its, normal_radii, estimate, (flags & 1) != 0};
  return 0;
}

// the raw clouds of a call on the device, and what the host knows of them
struct MsClouds {
  const float* pts[2]; const long long* off; const int* rows;
  std::vector<long long> n1, n2;
  bool by_rows;
};

struct MsDebugOut { float* cloud; double* mean; int32_t* vox; int32_t* cnt; int64_t* sizes; long long n; };

// pyramid, then the levels' ICP chained on the device; dbg: the pyramid alone, read back (one pair: the cloud against nothing)
int ms_run(alignnet_handle* h, const std::string& fn, const MsClouds& c, int B, const MsSchedule& s, const double* init, double* out, double* fitness,
           double* rmse, int32_t* iterations, int32_t* level_sizes, const MsDebugOut* dbg)
{
  const int L = s.L;
  long long total[2] = {0, 0};
  std::vector<long long> slot((size_t)B * 2);
  long long slot_total = 0, biggest = 0;
  for (int b = 0; b < B; ++b)
    for (int side = 0; side < 2; ++side) {
      const long long n = side ? c.n2[b] : c.n1[b];
      if (n > kMsMaxPoints) return fail(h, fn + ": more than 2^30 points in a cloud");
      slot[(size_t)b * 2 + side] = slot_total; slot_total += n; total[side] += n; biggest = std::max(biggest, n);
    }
  int ld_of[kMsMaxLevels], Ld = 0;
  MsArgs a;
  for (int l = 0; l < L; ++l) { ld_of[l] = -1; if (s.voxel[l] > 0.0) { ld_of[l] = Ld; a.voxel[Ld++] = s.voxel[l]; } }
  const size_t uB = (size_t)B, uLd = (size_t)Ld;
  MsCarve cv;
  const size_t o_key = cv.take(uLd * slot_total * 8), o_val = cv.take(uLd * slot_total * 4);
  const size_t o_p0 = cv.take(uLd * total[0] * 12), o_p1 = cv.take(uLd * total[1] * 12);
  const size_t o_slot = cv.take(uB * 2 * 8), o_cnt = cv.take(uLd * uB * 2 * 8), o_off = cv.take(uLd * (uB + 1) * 2 * 8), o_err = cv.take(4);
  const size_t o_T = cv.take(2 * uB * 16 * 8), o_fr = cv.take(2 * uB * 8), o_it = cv.take((size_t)L * uB * 4), o_ws = cv.take((size_t)L * uB * 2 * 8);
  const size_t o_dm = dbg ? cv.take(uLd * total[0] * 24) : 0, o_dv = dbg ? cv.take(uLd * total[0] * 12) : 0, o_dc = dbg ? cv.take(uLd * total[0] * 4) : 0;
  if (grow_bytes(h, &h->multiscale_ws, &h->multiscale_ws_bytes, cv.bytes)) return 1;
  h->multiscale_ws_used = cv.bytes;
  char* const ws = static_cast<char*>(h->multiscale_ws);
  MsDrain drain{h->stream};

  a.pts[0] = c.pts[0]; a.pts[1] = c.pts[1]; a.off = c.off; a.rows = c.rows; a.B = B; a.Ld = Ld;
  a.slot = reinterpret_cast<long long*>(ws + o_slot); a.slot_total = slot_total;
  a.key = reinterpret_cast<unsigned long long*>(ws + o_key); a.val = reinterpret_cast<int*>(ws + o_val);
  a.cnt = reinterpret_cast<long long*>(ws + o_cnt); a.lvl_off = reinterpret_cast<long long*>(ws + o_off);
  a.lvl_pts[0] = reinterpret_cast<float*>(ws + o_p0); a.lvl_pts[1] = reinterpret_cast<float*>(ws + o_p1);
  a.total[0] = total[0]; a.total[1] = total[1];
  a.err = reinterpret_cast<int*>(ws + o_err);
  a.dbg_mean = dbg ? reinterpret_cast<double*>(ws + o_dm) : nullptr;
  a.dbg_vox = dbg ? reinterpret_cast<int*>(ws + o_dv) : nullptr;
  a.dbg_cnt = dbg ? reinterpret_cast<int*>(ws + o_dc) : nullptr;

  std::vector<long long> h_off(uLd * (uB + 1) * 2);
  if (Ld) {
    int h_err = 0;
    HIP_TRY(h, hipMemcpyAsync(ws + o_slot, slot.data(), uB * 2 * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(a.err, 0, 4, h->stream));
    static alignnet::PerDeviceOnce attr;
    if (attr.need(h->cfg.device)) {
      HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(ms_sort_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMsChunk * 12 + kMsScratch));
      attr.mark(h->cfg.device);
    }
    int P = 1;
    while (P < biggest) P <<= 1;
    const size_t lds = (size_t)std::min(P, kMsChunk) * 12 + kMsScratch;   // sized by the call's largest cloud
    {
      alignnet::ProfScope prof_scope(h, alignnet::PK_ICP_PYRAMID);
      hipLaunchKernelGGL(ms_sort_kernel, dim3(2 * B, Ld), dim3(kMsThreads), lds, h->stream, a);
      hipLaunchKernelGGL(ms_scan_kernel, dim3(2, Ld), dim3(64), 0, h->stream, a);
      hipLaunchKernelGGL(ms_emit_kernel, dim3(2 * B, Ld), dim3(kMsThreads), 0, h->stream, a);
    }
    HIP_TRY(h, hipGetLastError());
    // the levels' sizes (launch geometry, search choice and workspace of the ICP) and the error flag: the call's first synchronisation
    HIP_TRY(h, hipMemcpyAsync(h_off.data(), a.lvl_off, h_off.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&h_err, a.err, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h_err) return fail(h, fn + ": a cloud is wider than 2^21 voxels on an axis at one of the voxel sizes, or holds a coordinate that is not finite");
  }
  // sizes of (level, pair, side)
  std::vector<std::vector<long long>> n1(L), n2(L);
  for (int l = 0; l < L; ++l) {
    if (ld_of[l] < 0) { n1[l] = c.n1; n2[l] = c.n2; continue; }
    const long long* t = h_off.data() + (size_t)ld_of[l] * (uB + 1) * 2;
    n1[l].resize(B); n2[l].resize(B);
    for (int b = 0; b < B; ++b) { n1[l][b] = t[(b + 1) * 2] - t[b * 2]; n2[l][b] = t[(b + 1) * 2 + 1] - t[b * 2 + 1]; }
  }
  if (level_sizes)
    for (int b = 0; b < B; ++b)
      for (int l = 0; l < L; ++l) { level_sizes[((size_t)b * L + l) * 2] = (int32_t)n1[l][b]; level_sizes[((size_t)b * L + l) * 2 + 1] = (int32_t)n2[l][b]; }

  if (dbg) {   // one cloud: per level [n] slots of the caller's arrays, the level's size in sizes[l]
    const size_t n = (size_t)dbg->n;
    for (int l = 0; l < L; ++l) {
      const int d = ld_of[l];
      dbg->sizes[l] = n1[l][0];
      const size_t m = (size_t)n1[l][0];
      if (d < 0 || !m) continue;   // (a raw level is the caller's own cloud)
      HIP_TRY(h, hipMemcpyAsync(dbg->cloud + l * n * 3, a.lvl_pts[0] + d * n * 3, m * 12, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipMemcpyAsync(dbg->mean + l * n * 3, a.dbg_mean + d * n * 3, m * 24, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipMemcpyAsync(dbg->vox + l * n * 3, a.dbg_vox + d * n * 3, m * 12, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipMemcpyAsync(dbg->cnt + l * n, a.dbg_cnt + d * n, m * 4, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    drain.armed = false;
    return 0;
  }

  // the levels: level l reads the transform level l - 1 wrote and writes the one level l + 1 reads; nothing comes to the host in between
  double* const T = reinterpret_cast<double*>(ws + o_T);
  double* const fr = reinterpret_cast<double*>(ws + o_fr);
  int* const it = reinterpret_cast<int*>(ws + o_it);
  long long* const ws_off = reinterpret_cast<long long*>(ws + o_ws);
  HIP_TRY(h, hipMemcpyAsync(T, init, uB * 16 * 8, hipMemcpyHostToDevice, h->stream));
  std::vector<std::vector<long long>> h_ws_off(L);
  for (int l = 0; l < L; ++l) {
    const int d = ld_of[l];
    const float* pts[2] = {c.pts[0], c.pts[1]};
    const long long* off = c.off; const int* rows = c.rows;
    long long stage_n2 = c.by_rows ? 0 : *std::max_element(n2[l].begin(), n2[l].end());
    if (d >= 0) {
      pts[0] = a.lvl_pts[0] + (size_t)d * total[0] * 3; pts[1] = a.lvl_pts[1] + (size_t)d * total[1] * 3;
      off = a.lvl_off + (size_t)d * (uB + 1) * 2; rows = nullptr;
      stage_n2 = *std::max_element(n2[l].begin(), n2[l].end());
    }
    const alignnet::IcpDeviceIo io = {T + (size_t)(l & 1) * uB * 16, T + (size_t)((l + 1) & 1) * uB * 16, fr, fr + B, it + (size_t)l * uB,
                                      ws_off + (size_t)l * uB * 2, &h_ws_off[l]};
    if (alignnet_icp_run_device(h, pts, off, rows, n1[l].data(), n2[l].data(), stage_n2, B, io, s.radius[l], s.normal_radius ? s.normal_radius[l] : 0.0,
                                s.its[l], s.full, s.estimate))
      return 1;
  }
  std::vector<int> h_it((size_t)L * uB);
  HIP_TRY(h, hipMemcpyAsync(out, T + (size_t)(L & 1) * uB * 16, uB * 16 * 8, hipMemcpyDeviceToHost, h->stream));
  if (fitness) HIP_TRY(h, hipMemcpyAsync(fitness, fr, uB * 8, hipMemcpyDeviceToHost, h->stream));
  if (rmse) HIP_TRY(h, hipMemcpyAsync(rmse, fr + B, uB * 8, hipMemcpyDeviceToHost, h->stream));
  if (iterations) HIP_TRY(h, hipMemcpyAsync(h_it.data(), it, h_it.size() * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));   // the call's second and last synchronisation
  drain.armed = false;
  if (iterations)
    for (int b = 0; b < B; ++b)
      for (int l = 0; l < L; ++l) iterations[(size_t)b * L + l] = h_it[(size_t)l * uB + b];
  return 0;
}

}  // namespace

void alignnet_multiscale_free(alignnet_handle* h)
{
  if (!h || !h->multiscale_ws) return;
  hipFree(h->multiscale_ws);
  h->multiscale_ws = nullptr; h->multiscale_ws_bytes = 0; h->multiscale_ws_used = 0;
}

extern "C" int alignnet_icp_multiscale_register(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets, int32_t B,
                                                const double* init, int32_t L, const double* voxel_sizes, const double* radii, const int32_t* its,
                                                const double* normal_radii, int32_t estimate, int32_t flags, double* out, double* fitness, double* rmse,
                                                int32_t* iterations, int32_t* level_sizes)
{
  if (!h) return 1;
  const std::string fn("alignnet_icp_multiscale_register");
  MsSchedule s;
  if (ms_schedule(h, fn, L, voxel_sizes, radii, its, normal_radii, estimate, flags, &s)) return 1;
  if (!init || !out) return fail(h, fn + ": null init / out");
  PairUpload up;
  if (upload_pairs(h, fn, points1, points2, offsets, B, &up)) return 1;
  MsClouds c{{up.pts[0].p, up.pts[1].p}, up.off.p, nullptr, up.n1, up.n2, false};
  return ms_run(h, fn, c, B, s, init, out, fitness, rmse, iterations, level_sizes, nullptr);
}

extern "C" int alignnet_icp_multiscale_register_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, const double* init, int32_t L,
                                                        const double* voxel_sizes, const double* radii, const int32_t* its, const double* normal_radii,
                                                        int32_t estimate, int32_t flags, double* out, double* fitness, double* rmse, int32_t* iterations,
                                                        int32_t* level_sizes)
{
  if (!h) return 1;
  const std::string fn("alignnet_icp_multiscale_register_dataset");
  MsSchedule s;
  if (ms_schedule(h, fn, L, voxel_sizes, radii, its, normal_radii, estimate, flags, &s)) return 1;
  if (!init || !out) return fail(h, fn + ": null init / out");
  alignnet::DatasetTables t;
  if (!alignnet_dataset_tables(h, &t)) return fail(h, fn + ": no dataset uploaded");
  if (!rows || B < 1) return fail(h, fn + ": null rows or B < 1");
  for (int i = 0; i < B; ++i)
    if (rows[i] < 0 || rows[i] >= t.n) return fail(h, fn + ": row " + std::to_string(rows[i]) + " out of range");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  DevBuf<int> d_rows;
  HIP_TRY(h, d_rows.alloc((size_t)B));
  HIP_TRY(h, hipMemcpyAsync(d_rows.p, rows, (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  MsClouds c{{t.pts[0], t.pts[1]}, t.off, d_rows.p, std::vector<long long>(B), std::vector<long long>(B), true};
  for (int i = 0; i < B; ++i) {
    c.n1[i] = t.h_off[((size_t)rows[i] + 1) * 2] - t.h_off[(size_t)rows[i] * 2];
    c.n2[i] = t.h_off[((size_t)rows[i] + 1) * 2 + 1] - t.h_off[(size_t)rows[i] * 2 + 1];
  }
  const int rc = ms_run(h, fn, c, B, s, init, out, fitness, rmse, iterations, level_sizes, nullptr);
  if (rc) hipStreamSynchronize(h->stream);   // (the rows' copy was queued from the caller's array)
  return rc;
}

extern "C" int alignnet_debug_voxel_pyramid(alignnet_handle* h, const float* points, int64_t n, int32_t L, const double* voxel_sizes, float* cloud,
                                            double* means, int32_t* voxels, int32_t* counts, int64_t* sizes)
{
  if (!h) return 1;
  const std::string fn("alignnet_debug_voxel_pyramid");
  if (L < 1 || L > kMsMaxLevels) return fail(h, fn + ": L must be in [1, " + std::to_string(kMsMaxLevels) + "], got " + std::to_string(L));
  if (!voxel_sizes || !cloud || !means || !voxels || !counts || !sizes) return fail(h, fn + ": null voxel_sizes or output");
  if (n < 0 || n > kMsMaxPoints) return fail(h, fn + ": n out of range");
  for (int l = 0; l < L; ++l)
    if (!std::isfinite(voxel_sizes[l])) return fail(h, fn + ": voxel_sizes[" + std::to_string(l) + "] is not finite");
  const int64_t off[4] = {0, 0, n, 0};
  PairUpload up;
  if (upload_pairs(h, fn, points, nullptr, off, 1, &up)) return 1;
  MsClouds c{{up.pts[0].p, up.pts[1].p}, up.off.p, nullptr, up.n1, up.n2, false};
  const MsSchedule s{L, voxel_sizes, nullptr, nullptr, nullptr, 1, false};
  const MsDebugOut d{cloud, means, voxels, counts, sizes, n};
  return ms_run(h, fn, c, 1, s, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &d);
}
