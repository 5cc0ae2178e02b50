// Host-side helpers that every stage file (alignnet_*.hip) shares: error reporting, device allocations and the upload of a call's clouds.
// Internal linkage throughout: a file uses whichever part it needs.
#pragma once
#include "engine.h"
#include <algorithm>

static inline int fail(const alignnet_handle* h, const std::string& m) { h->err = m; return 1; }

#define HIP_TRY(h, expr)                                                                         \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) return fail(h, std::string(#expr) + ": " + hipGetErrorString(e_));     \
  } while (0)

// a device allocation of one call: freed on every way out of it
template <class T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) hipFree(p); }
  hipError_t alloc(size_t n) { return hipMalloc(&p, n * sizeof(T)); }
};

// an array of the handle's that is kept between calls: at least max(need, 1) elements after this (contents are not kept when it grows)
template <typename T>
static int grow(alignnet_handle* h, T** p, size_t* cap, size_t need)
{
  if (need <= *cap && *p) return 0;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (*p) hipFree(*p);
  *p = nullptr; *cap = 0;
  HIP_TRY(h, hipMalloc(p, std::max<size_t>(need, 1) * sizeof(T)));
  *cap = std::max<size_t>(need, 1);
  return 0;
}

// a byte workspace of the handle's that the calls carve: at least `need` bytes after this.  The stream is drained before a smaller one is freed
static inline int grow_bytes(alignnet_handle* h, void** ws, size_t* bytes, size_t need)
{
  if (*bytes >= need) return 0;
  if (*ws) { HIP_TRY(h, hipStreamSynchronize(h->stream)); hipFree(*ws); *ws = nullptr; *bytes = 0; }
  HIP_TRY(h, hipMalloc(ws, need));
  *bytes = need;
  return 0;
}

// the clouds of a call that passes them from the host: two point blobs [n][3] float32 and the offsets table [B + 1][2], on the device until
// this goes out of scope; n1 / n2: the cloud sizes of the B pairs
struct PairUpload {
  DevBuf<float> pts[2]; DevBuf<long long> off;
  std::vector<long long> n1, n2;
};

// checks the offsets and the blobs, allocates and queues the three copies on h->stream; `name` is the entry point's in the messages
static inline int upload_pairs(alignnet_handle* h, const std::string& name, const float* points1, const float* points2, const int64_t* offsets, int32_t B,
                               PairUpload* u)
{
  static_assert(sizeof(long long) == sizeof(int64_t), "offsets");
  if (!offsets || B < 1) return fail(h, name + ": null offsets or B < 1");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  u->n1.resize(B); u->n2.resize(B);
  for (int i = 0; i < B; ++i) {
    u->n1[i] = offsets[(i + 1) * 2] - offsets[i * 2]; u->n2[i] = offsets[(i + 1) * 2 + 1] - offsets[i * 2 + 1];
    if (u->n1[i] < 0 || u->n2[i] < 0) return fail(h, name + ": offsets must be non-decreasing");
  }
  const size_t t0 = (size_t)offsets[B * 2], t1 = (size_t)offsets[B * 2 + 1];
  if ((t0 && !points1) || (t1 && !points2)) return fail(h, name + ": null point blob");
  HIP_TRY(h, u->pts[0].alloc(std::max<size_t>(t0, 1) * 3));
  HIP_TRY(h, u->pts[1].alloc(std::max<size_t>(t1, 1) * 3));
  HIP_TRY(h, u->off.alloc((size_t)(B + 1) * 2));
  if (t0) HIP_TRY(h, hipMemcpyAsync(u->pts[0].p, points1, t0 * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream));
  if (t1) HIP_TRY(h, hipMemcpyAsync(u->pts[1].p, points2, t1 * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(u->off.p, offsets, (size_t)(B + 1) * 2 * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  return 0;
}
