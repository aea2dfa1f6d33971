// sf_eplog_capi.cpp -- C ABI of the device-side episode log (include/sfmi.h, sf_episode_log.hip).
#include <memory>

#include "sf_batch.h"

struct sf_eplog {
  SfEplogArgs a{};  // (raw pointers into the buffers below: what the kernels get)
  int device = 0;
  DevBuf<int4> acc;
  DevBuf<sf_episode_record> ring;
  DevBuf<unsigned long long> hist;
  DevBuf<SfEplogHeader> hdr;
  DevBuf<uint32_t> counts, offs;
};

namespace {
size_t n_cells(const sf_eplog* h) { return (size_t)SF_EPLOG_ROWS * (size_t)((h->a.n + 255) / 256); }
}  // namespace

extern "C" int sf_eplog_create(int n_envs, int64_t capacity, int hist_lo, int hist_bins, int fire_action, int device,
                               sf_eplog** out) {
  if (!out || n_envs < 1 || n_envs > (1 << 26) || capacity < 1 || capacity > (1LL << 32) || hist_bins < 1 || hist_bins > 65536) {
    sf_set_error("sf_eplog_create: need 1 <= n_envs <= 2^26, 1 <= capacity <= 2^32 and 1 <= hist_bins <= 65536 "
                 "(got %d, %lld, %d)", n_envs, (long long)capacity, hist_bins);
    return SF_ERR_ARG;
  }
  *out = nullptr;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    sf_set_error("sf_eplog_create: no HIP device available; libsfmi has no CPU path");
    return SF_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= n_dev) {
    sf_set_error("sf_eplog_create: device %d out of range", device);
    return SF_ERR_ARG;
  }
  DeviceGuard guard(device);
  std::unique_ptr<sf_eplog> owner(new sf_eplog());  // (behind the guard: an error return frees what it holds)
  sf_eplog* const h = owner.get();
  h->device = device;
  h->a.n = n_envs;
  h->a.fire_action = fire_action;
  h->a.bins = hist_bins;
  h->a.hist_lo = hist_lo;
  h->a.capacity = (unsigned long long)capacity;
  HIP_TRY(h->acc.alloc((size_t)n_envs));
  HIP_TRY(h->ring.alloc((size_t)capacity));
  HIP_TRY(h->hist.alloc((size_t)hist_bins));
  HIP_TRY(h->hdr.alloc(1));
  HIP_TRY(h->counts.alloc(n_cells(h)));
  HIP_TRY(h->offs.alloc(n_cells(h)));
  h->a.acc = h->acc.get();
  h->a.ring = h->ring.get();
  h->a.hist = h->hist.get();
  h->a.hdr = h->hdr.get();
  h->a.counts = h->counts.get();
  h->a.offs = h->offs.get();
  HIP_TRY(hipMemset(h->a.acc, 0, sizeof(int4) * (size_t)n_envs));
  HIP_TRY(hipMemset(h->a.ring, 0, sizeof(sf_episode_record) * (size_t)capacity));
  HIP_TRY(hipMemset(h->a.hist, 0, sizeof(unsigned long long) * (size_t)hist_bins));
  HIP_TRY(hipMemset(h->a.hdr, 0, sizeof(SfEplogHeader)));
  HIP_TRY(hipDeviceSynchronize());
  *out = owner.release();
  return SF_OK;
}

extern "C" int sf_eplog_destroy(sf_eplog* h) {
  if (!h) return SF_OK;
  DeviceGuard guard(h->device);  // (in scope while the buffers are freed)
  delete h;
  return SF_OK;
}

extern "C" int sf_eplog_update(sf_eplog* h, const int32_t* rew_dev, const uint8_t* done_dev, const uint8_t* info_dev,
                               const void* actions_dev, int act_type, int K, void* stream) {
  if (!h || !rew_dev || !done_dev || !info_dev) {
    sf_set_error("sf_eplog_update: null log, rew, done or info");
    return SF_ERR_ARG;
  }
  if (K < 1) {
    sf_set_error("sf_eplog_update: K >= 1 rows (got %d)", K);
    return SF_ERR_ARG;
  }
  if (actions_dev && act_type != SF_ACT_U8 && act_type != SF_ACT_I32 && act_type != SF_ACT_I64) {
    sf_set_error("sf_eplog_update: act_type must be 1, 4 or 8 (got %d)", act_type);
    return SF_ERR_ARG;
  }
  DeviceGuard guard(h->device);
  HIP_TRY(sf_launch_eplog_update(h->a, rew_dev, done_dev, info_dev, actions_dev, act_type, K, (hipStream_t)stream));
  return SF_OK;
}

extern "C" int sf_eplog_restart(sf_eplog* h, void* stream) {
  if (!h) {
    sf_set_error("sf_eplog_restart: null log");
    return SF_ERR_ARG;
  }
  DeviceGuard guard(h->device);
  HIP_TRY(hipMemsetAsync(h->a.acc, 0, sizeof(int4) * (size_t)h->a.n, (hipStream_t)stream));
  return SF_OK;
}

extern "C" int sf_eplog_restart_where(sf_eplog* h, const uint8_t* mask_dev, void* stream) {
  if (!h || !mask_dev) {
    sf_set_error("sf_eplog_restart_where: null log or mask");
    return SF_ERR_ARG;
  }
  DeviceGuard guard(h->device);
  HIP_TRY(sf_launch_eplog_restart_where(h->a, mask_dev, (hipStream_t)stream));
  return SF_OK;
}

extern "C" int sf_eplog_clear(sf_eplog* h, void* stream) {
  if (!h) {
    sf_set_error("sf_eplog_clear: null log");
    return SF_ERR_ARG;
  }
  DeviceGuard guard(h->device);
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(h->a.acc, 0, sizeof(int4) * (size_t)h->a.n, st));
  HIP_TRY(hipMemsetAsync(h->a.ring, 0, sizeof(sf_episode_record) * (size_t)h->a.capacity, st));
  HIP_TRY(hipMemsetAsync(h->a.hist, 0, sizeof(unsigned long long) * (size_t)h->a.bins, st));
  HIP_TRY(hipMemsetAsync(h->a.hdr, 0, sizeof(SfEplogHeader), st));
  return SF_OK;
}

extern "C" int sf_eplog_read(sf_eplog* h, uint64_t* total, uint64_t* rows_seen, sf_episode_record* records_host,
                             int64_t* hist_host, void* stream) {
  if (!h) {
    sf_set_error("sf_eplog_read: null log");
    return SF_ERR_ARG;
  }
  DeviceGuard guard(h->device);
  hipStream_t st = (hipStream_t)stream;
  SfEplogHeader hd;
  HIP_TRY(hipMemcpyAsync(&hd, h->a.hdr, sizeof(hd), hipMemcpyDeviceToHost, st));
  if (records_host)
    HIP_TRY(hipMemcpyAsync(records_host, h->a.ring, sizeof(sf_episode_record) * (size_t)h->a.capacity, hipMemcpyDeviceToHost, st));
  if (hist_host)
    HIP_TRY(hipMemcpyAsync(hist_host, h->a.hist, sizeof(int64_t) * (size_t)h->a.bins, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (total) *total = hd.total;
  if (rows_seen) *rows_seen = hd.rows_seen;
  return SF_OK;
}
