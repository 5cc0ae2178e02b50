// One-call registration (include/alignnet_hip.h: alignnet_register / alignnet_register_dataset), gfx950 only.
//
// The evaluation loop joins the sampler, the eval forward, the yaw decode, get_mat_angle and the ICP refinement in host Python
// (train.py:447-481): eight tensors come down, three list comprehensions decode the yaws (models/tp8.py:55-65), get_mat_angle runs once per
// sample (evaluation.py:46-57) and the 4x4 inits go up again for the ICP call.  Here the same chain is queued on the handle's stream in one piece:
//   dataset_sample_kernel (alignnet_dataset.hip) -> the eval forward (alignnet_forward_device) -> register_decode_kernel -> register_init_kernel
//   -> [the loss of alignnet_eval_loss on the dataset's labels] -> [icp_kernel / icp_surface_kernel from the device-resident T_net] -> downloads
// and the host waits once, at the end.  Every buffer lives in RegisterWS on the handle: it grows when B grows (and, for clouds from the host, when
// they do), so a steady-state call allocates nothing.  The two kernels here are a few hundred flops per pair; what matters is that they are two
// launches between two latency-critical stages and that their fp64 arithmetic is NumPy's to the last bit (no contraction).
#include "engine.h"
#include "host_util.h"
#include <algorithm>
#include <cmath>
#include <vector>

namespace {

struct RegisterWS {
  int cap = 0;                       // pairs the buffers below hold
  float* f32 = nullptr;              // p[0] | p[1] [cap][N][3] | the eight outputs | labels [12][cap] | loss work
  float* p[2] = {nullptr, nullptr}; float* out[8] = {}; float* lab = nullptr; float* loss = nullptr;
  double* f64 = nullptr;             // angles [cap][4] | T_net [cap][16] | refined [cap][16] | fitness [cap] | rmse [cap]
  double *angles = nullptr, *tnet = nullptr, *refined = nullptr, *fit = nullptr, *rmse = nullptr;
  long long* i64 = nullptr;          // streams [cap] | ICP workspace offsets [2 cap] | offsets of host clouds [cap + 1][2]
  long long *streams = nullptr, *ws_off = nullptr, *off = nullptr;
  int* i32 = nullptr;                // rows [cap] | iterations [cap]
  int *rows = nullptr, *iters = nullptr;
  float* cloud[2] = {nullptr, nullptr};   // clouds from the host, each grown on its own
  size_t cloud_cap[2] = {0, 0};           // points
  std::vector<long long> h_ws_off, h_n1, h_n2;  // host staging that must outlive the queued copies
};

RegisterWS* rws(alignnet_handle* h) { return static_cast<RegisterWS*>(h->register_ws); }

void free_batch(RegisterWS* w)
{
  if (w->f32) hipFree(w->f32);
  if (w->f64) hipFree(w->f64);
  if (w->i64) hipFree(w->i64);
  if (w->i32) hipFree(w->i32);
  w->f32 = nullptr; w->f64 = nullptr; w->i64 = nullptr; w->i32 = nullptr; w->cap = 0;
}

size_t r64(size_t n) { return (n + 63) & ~(size_t)63; }   // carve in units of 64 elements

int ensure(alignnet_handle* h, int B)
{
  if (!h->register_ws) h->register_ws = new RegisterWS();
  RegisterWS* w = rws(h);
  if (B <= w->cap) return 0;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  free_batch(w);
  const size_t N = (size_t)h->cfg.num_points, nb2 = 2 * (size_t)h->cfg.num_bins, b = (size_t)B;
  const size_t widths[8] = {3, nb2, 3, 3, 3, 3, nb2, nb2};
  size_t nf = 2 * r64(b * N * 3) + r64(b * 12) + r64(alignnet_eval_loss_work_floats(B));
  for (int i = 0; i < 8; ++i) nf += r64(b * widths[i]);
  HIP_TRY(h, hipMalloc(&w->f32, nf * sizeof(float)));
  HIP_TRY(h, hipMalloc(&w->f64, (r64(b * 4) + 2 * r64(b * 16) + 2 * r64(b)) * sizeof(double)));
  HIP_TRY(h, hipMalloc(&w->i64, (r64(b) + r64(2 * b) + r64((b + 1) * 2)) * sizeof(long long)));
  HIP_TRY(h, hipMalloc(&w->i32, 2 * r64(b) * sizeof(int)));
  float* f = w->f32;
  for (int t = 0; t < 2; ++t) { w->p[t] = f; f += r64(b * N * 3); }
  for (int i = 0; i < 8; ++i) { w->out[i] = f; f += r64(b * widths[i]); }
  w->lab = f; f += r64(b * 12);
  w->loss = f;
  double* d = w->f64;
  w->angles = d; d += r64(b * 4);
  w->tnet = d; d += r64(b * 16);
  w->refined = d; d += r64(b * 16);
  w->fit = d; d += r64(b);
  w->rmse = d;
  w->streams = w->i64; w->ws_off = w->streams + r64(b); w->off = w->ws_off + r64(2 * b);
  w->rows = w->i32; w->iters = w->rows + r64(b);
  w->cap = B;
  return 0;
}

int ensure_cloud(alignnet_handle* h, int t, size_t points)
{
  RegisterWS* w = rws(h);
  if (points <= w->cloud_cap[t] && w->cloud[t]) return 0;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (w->cloud[t]) hipFree(w->cloud[t]);
  w->cloud[t] = nullptr; w->cloud_cap[t] = 0;
  const size_t cap = std::max<size_t>(points, 1);
  HIP_TRY(h, hipMalloc(&w->cloud[t], cap * 3 * sizeof(float)));
  w->cloud_cap[t] = cap;
  return 0;
}

// models/tp8.py:55-65 for one row of 2 nb logits, in NumPy's arithmetic: int64 class * float64 k, + the float32 residual widened, and the wrap.
// No contraction: a fused class * k + residual differs from NumPy's two roundings in the last bit.
__device__ __forceinline__ double register_decode_one(const float* __restrict__ L, int nb, double k, double pi, double two_pi)
{
#pragma clang fp contract(off)
  int cls = 0;
  float best = L[0];
  for (int j = 1; j < nb; ++j) {   // np.argmax: the FIRST maximum; a NaN counts as the maximum
    const float v = L[j];
    if (v > best || (v != v && best == best)) { best = v; cls = j; }
  }
  const double prod = (double)cls * k;
  double angle = prod + (double)L[nb + cls];
  if (angle > pi) angle = angle - two_pi;
  return angle;
}

// four lanes per pair: lane 0 decodes pc1's yaw, lane 1 pc2's, lane 2 the remaining angle; lane 0 collects them.  16 pairs per wave-sized workgroup.
// angles [B][4] = a1, a2, a_rem, pred_angle = (a2 - a1) + a_rem (train.py:456, in that order)
__global__ __launch_bounds__(64) void register_decode_kernel(const float* __restrict__ l1, const float* __restrict__ l2, const float* __restrict__ lr,
                                                             int B, int nb, double k, double pi, double two_pi, double* __restrict__ angles)
{
#pragma clang fp contract(off)
  const int pair = blockIdx.x * 16 + (threadIdx.x >> 2), s = threadIdx.x & 3;
  const int b = min(pair, B - 1);   // (lanes past the batch run along on its last pair: the shuffles want every lane)
  double a = 0.0;
  if (s < 3) a = register_decode_one((s == 0 ? l1 : s == 1 ? l2 : lr) + (size_t)b * 2 * nb, nb, k, pi, two_pi);
  const int base = threadIdx.x & ~3;
  const double a1 = __shfl(a, base), a2 = __shfl(a, base + 1), ar = __shfl(a, base + 2);
  if (s == 0 && pair < B) {
    const double d = a2 - a1;
    double* o = angles + (size_t)pair * 4;
    o[0] = a1; o[1] = a2; o[2] = ar; o[3] = d + ar;
  }
}

// evaluation.py:46-57 get_mat_angle(t, angle, rotation_center = c) = Tr(c + t) Rz(angle) Tr(-c), the products in the order the two 4x4 matrix
// products take them: column 3 of Rz Tr(-c) is R (-c), then c + t is added.  One pair per lane; T [B][16] row-major
__global__ __launch_bounds__(64) void register_init_kernel(const float* __restrict__ trans, const float* __restrict__ center,
                                                           const double* __restrict__ angles, int B, double* __restrict__ T)
{
#pragma clang fp contract(off)
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double sn, cs;
  sincos(angles[(size_t)b * 4 + 3], &sn, &cs);
  const double cx = (double)center[b * 3], cy = (double)center[b * 3 + 1], cz = (double)center[b * 3 + 2];
  const double tx = (double)trans[b * 3], ty = (double)trans[b * 3 + 1], tz = (double)trans[b * 3 + 2];
  const double mx = -cx, my = -cy, mz = -cz, ms = -sn;
  const double rx = cs * mx + ms * my, ry = sn * mx + cs * my;
  double* o = T + (size_t)b * 16;
  o[0] = cs;  o[1] = ms;  o[2] = 0.0;  o[3] = rx + (cx + tx);
  o[4] = sn;  o[5] = cs;  o[6] = 0.0;  o[7] = ry + (cy + ty);
  o[8] = 0.0; o[9] = 0.0; o[10] = 1.0; o[11] = mz + (cz + tz);
  o[12] = 0.0; o[13] = 0.0; o[14] = 0.0; o[15] = 1.0;
}

int check_options(alignnet_handle* h, const std::string& name, const alignnet_register_options* o, const alignnet_register_outputs* out, bool dataset)
{
  if (!o || !out) return fail(h, name + ": null options / outputs");
  if (!out->transforms) return fail(h, name + ": outputs->transforms must not be null");
  if (o->refine < 0 || o->refine == 3 || o->refine > 4)
    return fail(h, name + ": refine must be 0 (none), 1 (point-to-point), 2 (point-to-plane) or 4 (generalized), got " + std::to_string(o->refine));
  if (o->its < 0) return fail(h, name + ": its must be >= 0");
  if (o->flags & ~ALIGNNET_ICP_FULL_ROTATION) return fail(h, name + ": unknown flags " + std::to_string(o->flags) + " (ALIGNNET_ICP_FULL_ROTATION is the only one)");
  if (o->refine == 0) {
    if (o->its != 0) return fail(h, name + ": its must be 0 without refinement");
    if (out->fitness || out->rmse || out->iterations) return fail(h, name + ": fitness / rmse / iterations are results of the refinement (refine is 0)");
  } else {
    if (!(o->radius > 0.0)) return fail(h, name + ": radius must be > 0");
    if (o->refine >= 2 && !(o->normal_radius > 0.0)) return fail(h, name + ": normal_radius must be > 0");
  }
  if (out->loss && !dataset) return fail(h, name + ": loss needs the dataset's labels (alignnet_register_dataset)");
  return 0;
}

// everything behind the staging: src names the clouds on the device, n1 / n2 the B source / target sizes, stage_n2 the ICP scan's LDS stage (<= 0: its budget)
int run(alignnet_handle* h, const alignnet::SampleSource& src, const long long* n1, const long long* n2, long long stage_n2, int B, uint64_t seed,
        const alignnet_register_options* o, const alignnet_register_outputs* out)
{
  RegisterWS* w = rws(h);
  alignnet_labels lab;
  if (alignnet_dataset_sample_launch(h, src, B, w->cap, seed, w->p[0], w->p[1], w->lab, &lab)) return 1;
  const alignnet_outputs d{w->out[0], w->out[1], w->out[2], w->out[3], w->out[4], w->out[5], w->out[6], w->out[7]};
  if (alignnet_forward_device(h, w->p[0], w->p[1], B, &d)) return 1;
  const int nb = h->cfg.num_bins;
  const double two_pi = 2.0 * M_PI, k = two_pi / (double)nb;   // 2 * np.pi / float(num_bins)
  hipLaunchKernelGGL(register_decode_kernel, dim3((B + 15) / 16), dim3(64), 0, h->stream, w->out[6], w->out[7], w->out[1], B, nb, k, (double)M_PI, two_pi,
                     w->angles);
  hipLaunchKernelGGL(register_init_kernel, dim3((B + 63) / 64), dim3(64), 0, h->stream, w->out[0], w->out[4], w->angles, B, w->tnet);
  HIP_TRY(h, hipGetLastError());
  if (out->loss && alignnet_eval_loss_launch(h, &lab, B, w->loss)) return 1;
  if (o->refine) {
    const alignnet::IcpDeviceIo io = {w->tnet, w->refined, w->fit, w->rmse, w->iters, w->ws_off, &w->h_ws_off};
    if (alignnet_icp_run_device(h, src.pts, src.off, src.rows, n1, n2, stage_n2, B, io, o->radius, o->normal_radius, o->its,
                                (o->flags & ALIGNNET_ICP_FULL_ROTATION) != 0, o->refine))
      return 1;
  }
  // downloads, then the call's one synchronisation
  const size_t b = (size_t)B;
  HIP_TRY(h, hipMemcpyAsync(out->transforms, o->refine ? w->refined : w->tnet, b * 16 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (out->network_transforms) HIP_TRY(h, hipMemcpyAsync(out->network_transforms, w->tnet, b * 16 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (out->angles) HIP_TRY(h, hipMemcpyAsync(out->angles, w->angles, b * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (out->fitness) HIP_TRY(h, hipMemcpyAsync(out->fitness, w->fit, b * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (out->rmse) HIP_TRY(h, hipMemcpyAsync(out->rmse, w->rmse, b * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (out->iterations) HIP_TRY(h, hipMemcpyAsync(out->iterations, w->iters, b * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (out->loss) HIP_TRY(h, hipMemcpyAsync(out->loss, w->loss, 17 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (out->net) {
    float* const host[8] = {out->net->pred_translations, out->net->pred_remaining_angle_logits, out->net->pred_s1_pc1centers, out->net->pred_s1_pc2centers,
                            out->net->pred_s2_pc1centers, out->net->pred_s2_pc2centers, out->net->pred_pc1angle_logits, out->net->pred_pc2angle_logits};
    const size_t nb2 = 2 * (size_t)nb;
    const size_t widths[8] = {3, nb2, 3, 3, 3, 3, nb2, nb2};
    for (int i = 0; i < 8; ++i)
      if (host[i]) HIP_TRY(h, hipMemcpyAsync(host[i], w->out[i], b * widths[i] * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return 0;
}

}  // namespace

void alignnet_register_free(alignnet_handle* h)
{
  if (!h || !h->register_ws) return;
  RegisterWS* w = rws(h);
  free_batch(w);
  for (int t = 0; t < 2; ++t) if (w->cloud[t]) hipFree(w->cloud[t]);
  delete w;
  h->register_ws = nullptr;
}

extern "C" int alignnet_register_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, uint64_t seed, const alignnet_register_options* options,
                                         const alignnet_register_outputs* outputs)
{
  if (!h) return 1;
  const std::string name("alignnet_register_dataset");
  if (check_options(h, name, options, outputs, true)) return 1;
  alignnet::DatasetTables t;
  if (!alignnet_dataset_tables(h, &t)) return fail(h, name + ": no dataset uploaded");
  if (!rows || B < 1) return fail(h, name + ": null rows or B < 1");
  for (int i = 0; i < B; ++i)
    if (rows[i] < 0 || rows[i] >= t.n) return fail(h, name + ": row " + std::to_string(rows[i]) + " out of range");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  if (ensure(h, B)) return 1;
  RegisterWS* w = rws(h);
  HIP_TRY(h, hipMemcpyAsync(w->rows, rows, (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  w->h_n1.resize(B); w->h_n2.resize(B);
  for (int i = 0; i < B; ++i) {
    w->h_n1[i] = t.h_off[((size_t)rows[i] + 1) * 2] - t.h_off[(size_t)rows[i] * 2];
    w->h_n2[i] = t.h_off[((size_t)rows[i] + 1) * 2 + 1] - t.h_off[(size_t)rows[i] * 2 + 1];
  }
  const alignnet::SampleSource src = {{t.pts[0], t.pts[1]}, t.off, t.labels, w->rows, nullptr};
  return run(h, src, w->h_n1.data(), w->h_n2.data(), 0, B, seed, options, outputs);
}

extern "C" int alignnet_register(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets, int32_t B, uint64_t seed,
                                 const int64_t* streams, const alignnet_register_options* options, const alignnet_register_outputs* outputs)
{
  if (!h) return 1;
  const std::string name("alignnet_register");
  if (check_options(h, name, options, outputs, false)) return 1;
  if (!offsets || B < 1) return fail(h, name + ": null offsets or B < 1");
  if (offsets[0] < 0 || offsets[1] < 0) return fail(h, name + ": offsets must not be negative");
  for (int i = 0; i < B; ++i)
    if (offsets[(i + 1) * 2] < offsets[i * 2] || offsets[(i + 1) * 2 + 1] < offsets[i * 2 + 1]) return fail(h, name + ": offsets must be non-decreasing");
  const size_t np[2] = {(size_t)offsets[B * 2], (size_t)offsets[B * 2 + 1]};
  if ((np[0] && !points1) || (np[1] && !points2)) return fail(h, name + ": null point blob");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  if (ensure(h, B) || ensure_cloud(h, 0, np[0]) || ensure_cloud(h, 1, np[1])) return 1;
  RegisterWS* w = rws(h);
  const float* const host[2] = {points1, points2};
  for (int t = 0; t < 2; ++t)
    if (np[t]) HIP_TRY(h, hipMemcpyAsync(w->cloud[t], host[t], np[t] * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(w->off, offsets, (size_t)(B + 1) * 2 * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  if (streams) HIP_TRY(h, hipMemcpyAsync(w->streams, streams, (size_t)B * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  w->h_n1.resize(B); w->h_n2.resize(B);
  for (int i = 0; i < B; ++i) { w->h_n1[i] = offsets[(i + 1) * 2] - offsets[i * 2]; w->h_n2[i] = offsets[(i + 1) * 2 + 1] - offsets[i * 2 + 1]; }
  const alignnet::SampleSource src = {{w->cloud[0], w->cloud[1]}, w->off, nullptr, nullptr, streams ? w->streams : nullptr};
  return run(h, src, w->h_n1.data(), w->h_n2.data(), *std::max_element(w->h_n2.begin(), w->h_n2.end()), B, seed, options, outputs);
}
