// sf_norm_capi.cpp -- C ABI of the device-side VecNormalize (include/sfmi.h, sf_normalize.hip).
#include <memory>
#include <vector>

#include "sf_batch.h"

struct sf_normalizer {
  sf_normalizer_params p{};
  int parity = 0;
  DevBuf<double> d_ret;       // per-env discounted return (VecNormalize.ret)
  DevBuf<double> d_partials;  // SF_NORM_GROUPS x 2 * (D + 1), then the ticket counter
  DevBuf<double> d_stats[2];  // 2 * D + 4
};

namespace {
// A call that updates the statistics flips z->parity on the host: a captured graph would replay the launch with the
// buffers of the capture, not of the replay (sfmi.h).  Such a call inside a capture is refused before anything is launched.
int refuse_in_capture(const char* who, hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  HIP_TRY(hipStreamIsCapturing(st, &cs));
  if (cs != hipStreamCaptureStatusNone) {
    sf_set_error("%s: a call that updates the running statistics cannot be captured in a HIP graph (the statistics' double "
                 "buffer flips on the host at every such call); capture frozen calls only", who);
    return SF_ERR_ARG;
  }
  return SF_OK;
}

int n_stats(const sf_normalizer* z) { return 2 * z->p.obs_dim + 4; }
int n_sums(const sf_normalizer* z) { return 2 * (z->p.obs_dim + 1); }
}  // namespace

extern "C" int sf_normalizer_create(const sf_normalizer_params* p, sf_normalizer** out) {
  if (!p || !out || p->n_envs <= 0 || p->obs_dim <= 0 || p->obs_dim > 24) {
    sf_set_error("sf_normalizer_create: need n_envs > 0 and 0 < obs_dim <= 24");
    return SF_ERR_ARG;
  }
  *out = nullptr;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    sf_set_error("sf_normalizer_create: no HIP device available; libsfmi has no CPU path");
    return SF_ERR_NO_DEVICE;
  }
  if (p->device_id < 0 || p->device_id >= n_dev) {
    sf_set_error("sf_normalizer_create: device_id %d out of range", p->device_id);
    return SF_ERR_ARG;
  }
  DeviceGuard guard(p->device_id);
  std::unique_ptr<sf_normalizer> owner(new sf_normalizer());  // (behind the guard: an error return frees what it holds)
  sf_normalizer* const z = owner.get();
  z->p = *p;
  // RunningMeanStd.__init__: mean 0, var 1, count 1e-4
  std::vector<double> st(n_stats(z), 0.0);
  for (int f = 0; f < p->obs_dim; f++) st[p->obs_dim + f] = 1.0;
  st[2 * p->obs_dim + 1] = 1.0;
  st[2 * p->obs_dim + 2] = st[2 * p->obs_dim + 3] = 1e-4;
  HIP_TRY(z->d_ret.alloc(p->n_envs));
  HIP_TRY(hipMemset(z->d_ret.get(), 0, sizeof(double) * p->n_envs));
  // rows of partial sums: SF_NORM_GROUPS from the stand-alone reduction, or one per wave of the step kernel
  // (sf_step_normalize; the batch is padded to whole workgroups of 256 envs)
  const size_t rows = (size_t)((p->n_envs + 255) / 256) * 4;
  const size_t prow = rows > SF_NORM_GROUPS ? rows : SF_NORM_GROUPS;
  HIP_TRY(z->d_partials.alloc(n_sums(z) * prow));
  HIP_TRY(hipMemset(z->d_partials.get(), 0, sizeof(double) * n_sums(z) * prow));
  for (int k = 0; k < 2; k++) {
    HIP_TRY(z->d_stats[k].alloc(n_stats(z)));
    HIP_TRY(hipMemcpy(z->d_stats[k].get(), st.data(), sizeof(double) * n_stats(z), hipMemcpyHostToDevice));
  }
  *out = owner.release();
  return SF_OK;
}

extern "C" int sf_normalizer_destroy(sf_normalizer* z) {
  if (!z) return SF_OK;
  DeviceGuard guard(z->p.device_id);  // (in scope while the buffers are freed)
  delete z;
  return SF_OK;
}

extern "C" int sf_normalize(sf_normalizer* z, const void* obs_dev, void* obs_out_dev, const int32_t* reward_dev,
                            float* reward_out_dev, int frozen, void* stream) {
  if (!z || (!obs_dev && !reward_dev)) {
    sf_set_error("sf_normalize: null normalizer or nothing to normalise");
    return SF_ERR_ARG;
  }
  if ((obs_dev == nullptr) != (obs_out_dev == nullptr) || (reward_dev == nullptr) != (reward_out_dev == nullptr)) {
    sf_set_error("sf_normalize: obs / reward inputs and outputs come in pairs");
    return SF_ERR_ARG;
  }
  DeviceGuard guard(z->p.device_id);
  const int k = z->parity;
  const int do_ob = (z->p.ob && obs_dev && !frozen) ? 1 : 0, do_ret = (z->p.ret && reward_dev && !frozen) ? 1 : 0;
  if (do_ob || do_ret) {
    const int rc = refuse_in_capture("sf_normalize", (hipStream_t)stream);
    if (rc != SF_OK) return rc;
  }
  HIP_TRY(sf_launch_normalize(z->p.ob ? obs_dev : nullptr, z->p.ob ? obs_out_dev : nullptr, z->p.obs_f64,
                              z->p.ret ? reward_dev : nullptr, z->p.ret ? reward_out_dev : nullptr, z->d_ret.get(), z->p.n_envs,
                              z->p.obs_dim, z->p.gamma, z->p.epsilon, z->p.clipob, z->p.cliprew, do_ob, do_ret,
                              z->d_partials.get(), z->d_stats[k].get(), z->d_stats[k ^ 1].get(), (hipStream_t)stream));
  if (do_ob || do_ret) z->parity = k ^ 1;
  return SF_OK;
}

extern "C" int sf_normalizer_get_state(sf_normalizer* z, double* host, double* ret_host, void* stream) {
  if (!z || !host) return SF_ERR_ARG;
  DeviceGuard guard(z->p.device_id);
  HIP_TRY(hipMemcpyAsync(host, z->d_stats[z->parity].get(), sizeof(double) * n_stats(z), hipMemcpyDeviceToHost, (hipStream_t)stream));
  if (ret_host)
    HIP_TRY(hipMemcpyAsync(ret_host, z->d_ret.get(), sizeof(double) * z->p.n_envs, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return SF_OK;
}

extern "C" int sf_normalizer_set_state(sf_normalizer* z, const double* host, const double* ret_host, void* stream) {
  if (!z || !host) return SF_ERR_ARG;
  DeviceGuard guard(z->p.device_id);
  HIP_TRY(hipMemcpyAsync(z->d_stats[z->parity].get(), host, sizeof(double) * n_stats(z), hipMemcpyHostToDevice, (hipStream_t)stream));
  if (ret_host)
    HIP_TRY(hipMemcpyAsync(z->d_ret.get(), ret_host, sizeof(double) * z->p.n_envs, hipMemcpyHostToDevice, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return SF_OK;
}

extern "C" int sf_step_normalize(sf_batch* b, sf_normalizer* z, const void* actions_dev, int act_type, void* obs_dev,
                                 int32_t* reward_dev, uint8_t* done_dev, uint8_t* info_dev, float* reward_out_dev, int frozen,
                                 void* stream) {
  if (!b || !z || !obs_dev || !reward_dev || !reward_out_dev) {
    sf_set_error("sf_step_normalize: null batch, normalizer, obs, reward or reward_out");
    return SF_ERR_ARG;
  }
  if (sf_n_envs(b) != z->p.n_envs || sf_obs_dim(b) != z->p.obs_dim) {
    sf_set_error("sf_step_normalize: the normalizer was made for %d envs x %d features", z->p.n_envs, z->p.obs_dim);
    return SF_ERR_ARG;
  }
  if (frozen) {
    int rc = sf_step(b, actions_dev, act_type, obs_dev, reward_dev, done_dev, info_dev, stream);
    if (rc != SF_OK) return rc;
    return sf_normalize(z, obs_dev, obs_dev, reward_dev, reward_out_dev, 1, stream);
  }
  DeviceGuard guard(z->p.device_id);
  int rows = 0;
  int rc = refuse_in_capture("sf_step_normalize", (hipStream_t)stream);
  if (rc != SF_OK) return rc;
  rc = sf_step_with_norm_partials(b, actions_dev, act_type, obs_dev, reward_dev, done_dev, info_dev, z->d_partials.get(),
                                      z->p.ret ? z->d_ret.get() : nullptr, z->p.gamma, &rows, stream);
  if (rc != SF_OK) return rc;
  const int k = z->parity;
  HIP_TRY(sf_launch_normalize_after_step(z->p.ob ? obs_dev : nullptr, z->p.ob ? obs_dev : nullptr, z->p.obs_f64,
                                         z->p.ret ? reward_dev : nullptr, z->p.ret ? reward_out_dev : nullptr, z->p.n_envs,
                                         z->p.obs_dim, z->p.epsilon, z->p.clipob, z->p.cliprew, z->p.ob, z->p.ret, z->d_partials.get(),
                                         rows, z->d_stats[k].get(), z->d_stats[k ^ 1].get(), (hipStream_t)stream));
  z->parity = k ^ 1;
  return SF_OK;
}
