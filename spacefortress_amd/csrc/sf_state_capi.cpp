// sf_state_capi.cpp -- the C ABI of include/sfmi.h, the host half of sf_state_ops.hip: field access with the missile slot
// view, and the lane states.  Host code only.
#include <string.h>

#include "sf_batch.h"

int sfb_flush_missile_view(sf_batch* b, hipStream_t stream) {
  if (!b->mslots_dirty) return SF_OK;
  HIP_TRY(sf_launch_slots_to_mpool(b->d_state.get(), b->args.lanes, b->n_envs, b->d_ms_pos.get(), b->d_ms_ang.get(), stream));
  b->mslots_dirty = false;
  b->draw_current = false;
  return SF_OK;
}

// ---- field access -------------------------------------------------------------------------

extern "C" int sf_n_fields(void) { return SF_F_COUNT; }

extern "C" int sf_field_info(int f, sf_field_desc* out) {
  if (f < 0 || f >= SF_F_COUNT || !out) {
    sf_set_error("sf_field_info: bad field id %d", f);
    return SF_ERR_FIELD;
  }
  out->name = sfl::kFields[f].name;
  out->elem_size = sfl::kFields[f].elem_size;
  out->count = sfl::kFields[f].count;
  out->is_float = sfl::kFields[f].is_float;
  return SF_OK;
}

extern "C" int sf_field_id(const char* name) {
  if (!name) return SF_ERR_FIELD;
  for (int f = 0; f < SF_F_COUNT; f++)
    if (!strcmp(name, sfl::kFields[f].name)) return f;
  sf_set_error("unknown field `%s'", name);
  return SF_ERR_FIELD;
}

// The tiled device layout never leaves the library: a small kernel gathers the field into (or
// scatters it from) a linear [count][n_envs] staging buffer, which is what the host sees.
static int field_copy(sf_batch* b, int f, void* host, size_t bytes, bool to_host) {
  if (!b || !host) return SF_ERR_ARG;
  if (f < 0 || f >= SF_F_COUNT) {
    sf_set_error("bad field id %d", f);
    return SF_ERR_FIELD;
  }
  const sfl::FieldMeta& m = sfl::kFields[f];
  const size_t total = (size_t)b->n_envs * m.elem_size * m.count;
  if (bytes != total) {
    sf_set_error("field %s: expected %zu bytes, got %zu", m.name, total, bytes);
    return SF_ERR_FIELD;
  }
  if (!to_host) SF_TRY(sf_field_values_fit(f, host, b->n_envs));
  DeviceGuard guard(b->device);
  HIP_TRY(hipDeviceSynchronize());
  const bool mview = m.kind == SF_FK_MPOOL;                      // missile_x / missile_y / missile_angle
  const bool mmask_write = f == SF_F_missile_mask && !to_host;   // which slots hold a missile
  if (mview || mmask_write) {
    // the per-slot view of the missiles: made on first use, refreshed from the pools unless it already holds edits
    const size_t cells = (size_t)b->n_envs * SF_NSLOT;
    if (!b->d_ms_pos) {
      HIP_TRY(b->d_ms_pos.alloc(cells * 16));
      HIP_TRY(b->d_ms_ang.alloc(cells));
    }
    if (!b->mslots_dirty) HIP_TRY(sf_launch_mpool_to_slots(b->d_state.get(), b->n_envs, b->d_ms_pos.get(), b->d_ms_ang.get(), nullptr));
  }
  if (!to_host) {
    HIP_TRY(hipMemcpy(b->d_scratch.get(), host, total, hipMemcpyHostToDevice));
    b->draw_current = false;
  }
  if (mview) {
    const int which = f == SF_F_missile_x ? 0 : (f == SF_F_missile_y ? 1 : 2);
    HIP_TRY(sf_launch_mslot_component(b->d_ms_pos.get(), b->d_ms_ang.get(), (long)b->n_envs * SF_NSLOT, which, b->d_scratch.get(),
                                      to_host ? 1 : 0, nullptr));
    if (!to_host) b->mslots_dirty = true;
  } else {
    HIP_TRY(sf_launch_field_copy(b->d_state.get(), b->n_envs, f, b->d_scratch.get(), to_host ? 1 : 0, nullptr));
    if (mmask_write) b->mslots_dirty = true;  // the pools follow the masks
  }
  HIP_TRY(hipDeviceSynchronize());
  if (to_host) HIP_TRY(hipMemcpy(host, b->d_scratch.get(), total, hipMemcpyDeviceToHost));
  // (a packed per-episode field rewritten with values that fit repairs THAT field; the sticky count of sf_check_state is not
  //  touched here -- other fields, other envs may have wrapped: sf_clear_state_errors, for a caller that has rewritten them all)
  return SF_OK;
}

extern "C" int sf_clear_state_errors(sf_batch* b) {
  if (!b) {
    sf_set_error("sf_clear_state_errors: null batch");
    return SF_ERR_ARG;
  }
  DeviceGuard guard(b->device);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(b->d_acc.get() + SF_ACC_OVERFLOW, 0, sizeof(unsigned long long)));
  return SF_OK;
}

// Diagnostics: move a known number of bytes with the step kernel's own access pattern (whole
// 16-byte chunks, 64-lane rows) so rocprofv3's FETCH_SIZE / WRITE_SIZE can be calibrated.
extern "C" int sf_calibration_copy(sf_batch* b, int which, size_t* bytes_moved) {
  if (!b) return SF_ERR_ARG;
  const int groups[2] = {SF_G_shell_pos, SF_G_missile_pos};
  if (which < 0 || which > 1) {
    sf_set_error("sf_calibration_copy: which must be 0 or 1");
    return SF_ERR_ARG;
  }
  DeviceGuard guard(b->device);
  const int g = groups[which];
  static_assert(sfl::kGroups[SF_G_shell_pos].chunk == 16 && sfl::kGroups[SF_G_missile_pos].chunk == 16, "chunk");
  HIP_TRY(sf_launch_group_copy(b->d_state.get(), b->n_envs, g, b->d_scratch.get(), nullptr));
  HIP_TRY(hipDeviceSynchronize());
  if (bytes_moved) *bytes_moved = (size_t)b->n_envs * sfl::kGroups[g].slots * 16;
  return SF_OK;
}

extern "C" int sf_get_field(sf_batch* b, int f, void* host, size_t bytes) {
  return field_copy(b, f, host, bytes, true);
}
extern "C" int sf_set_field(sf_batch* b, int f, const void* host, size_t bytes) {
  return field_copy(b, f, const_cast<void*>(host), bytes, false);
}

// One state field of every env into DEVICE memory, [count][n_envs] in the field's element type like sf_get_field's host
// layout, ordered on `stream` behind the steps issued there and without a synchronise or a PCIe copy: what on-device
// bookkeeping reads between two steps (spacefortress_amd/durations.py).  Not for the missile fields (their per-slot view is a
// host-side convenience made on demand: sf_get_field).
extern "C" int sf_get_field_dev(sf_batch* b, int f, void* dev, size_t bytes, void* stream) {
  if (!b || !dev || f < 0 || f >= SF_F_COUNT) {
    sf_set_error("sf_get_field_dev: bad argument (field %d)", f);
    return b && dev ? SF_ERR_FIELD : SF_ERR_ARG;
  }
  const sfl::FieldMeta& m = sfl::kFields[f];
  const size_t total = (size_t)b->n_envs * m.elem_size * m.count;
  if (bytes != total) {
    sf_set_error("field %s: expected %zu bytes, got %zu", m.name, total, bytes);
    return SF_ERR_FIELD;
  }
  if (m.kind == SF_FK_MPOOL) {
    sf_set_error("sf_get_field_dev: %s is a per-slot view of the tiles' missile pools: read it with sf_get_field", m.name);
    return SF_ERR_FIELD;
  }
  DeviceGuard guard(b->device);
  SF_FLUSH_VIEW(b, (hipStream_t)stream);
  HIP_TRY(sf_launch_field_copy(b->d_state.get(), b->n_envs, f, (unsigned char*)dev, 1, (hipStream_t)stream));
  return SF_OK;
}

// ---------------------------------------------------------------------------------------------
// lane states (sfmi.h): rows of SF_LANE_STATE_BYTES <-> lanes, on the device (sf_state_ops.hip: sf_lanes_*_kernel)
namespace {
void lane_header(const sf_batch* b, uint32_t h[4]) {
  h[0] = SF_LANE_STATE_MAGIC | SF_LANE_STATE_VERSION;
  h[1] = (b->autoturn ? 1u : 0u) | (b->preset.shaped ? 2u : 0u);
  h[2] = b->seed;
  h[3] = (uint32_t)b->spawn_len;
}
// SF_ACT_I32 -> 0, SF_ACT_I64 -> 1, else -1
int lane_idx64(int idx_type) { return idx_type == SF_ACT_I32 ? 0 : (idx_type == SF_ACT_I64 ? 1 : -1); }
int lane_args(const sf_batch* b, const void* lanes_dev, int idx_type, int n, const char* who) {
  if (!b || n < 0 || lane_idx64(idx_type) < 0) {
    sf_set_error("%s: needs a batch, n >= 0 and idx_type SF_ACT_I32 or SF_ACT_I64", who);
    return SF_ERR_ARG;
  }
  if (!lanes_dev && n > b->n_envs) {
    sf_set_error("%s: no lane list and n = %d > n_envs = %d", who, n, b->n_envs);
    return SF_ERR_ARG;
  }
  return SF_OK;
}
int lane_obs_ok(const sf_batch* b, const void* obs_dev, const char* who) {
  if (obs_dev && (sfb_is_image(b) || b->args.obs_type == SF_OBS_NONE)) {
    sf_set_error("%s: obs_dev is for the symbolic observation types; image batches draw with sf_render afterwards", who);
    return SF_ERR_ARG;
  }
  return SF_OK;
}
int load_rows(sf_batch* b, const void* lanes_dev, int idx64, int n, const void* rows_dev, long n_rows, const void* row_idx_dev,
              void* obs_dev, hipStream_t stream) {
  uint32_t h[4];
  lane_header(b, h);
  HIP_TRY(sf_launch_lanes_load(b->args, lanes_dev, idx64, n, (const unsigned char*)rows_dev, row_idx_dev, n_rows, h, b->d_lmap,
                               b->d_ltflag, b->d_ltlist, b->d_ltcount, b->d_lrefused, obs_dev, stream));
  b->draw_current = false;  // (the next frame rebuilds the draw records from the state: sf_drawrec_kernel)
  return SF_OK;
}
}  // namespace

extern "C" int sf_lane_state_bytes(void) { return SF_LANE_STATE_BYTES; }

extern "C" int sf_lane_state_header(const sf_batch* b, uint32_t* header) {
  if (!b || !header) {
    sf_set_error("sf_lane_state_header: null argument");
    return SF_ERR_ARG;
  }
  lane_header(b, header);
  return SF_OK;
}

extern "C" int sf_save_lanes(sf_batch* b, const void* lanes_dev, int idx_type, int n, void* rows_dev, void* stream) {
  int rc = lane_args(b, lanes_dev, idx_type, n, "sf_save_lanes");
  if (rc != SF_OK) return rc;
  if (n > 0 && !rows_dev) {
    sf_set_error("sf_save_lanes: null rows");
    return SF_ERR_ARG;
  }
  DeviceGuard guard(b->device);
  SF_FLUSH_VIEW(b, stream);
  uint32_t h[4];
  lane_header(b, h);
  HIP_TRY(sf_launch_lanes_save(b->d_state.get(), b->n_envs, lanes_dev, lane_idx64(idx_type), n, (unsigned char*)rows_dev, h, b->d_lrefused,
                               (hipStream_t)stream));
  return SF_OK;
}

extern "C" int sf_load_lanes(sf_batch* b, const void* lanes_dev, int idx_type, int n, const void* rows_dev, int n_rows,
                             const void* row_idx_dev, void* obs_dev, void* stream) {
  int rc = lane_args(b, lanes_dev, idx_type, n, "sf_load_lanes");
  if (rc == SF_OK) rc = lane_obs_ok(b, obs_dev, "sf_load_lanes");
  if (rc != SF_OK) return rc;
  if (n_rows < 0 || (n > 0 && (!rows_dev || n_rows == 0))) {
    sf_set_error("sf_load_lanes: needs rows (n_rows = %d)", n_rows);
    return SF_ERR_ARG;
  }
  if (!row_idx_dev && n > n_rows) {
    sf_set_error("sf_load_lanes: no row list and n = %d > n_rows = %d", n, n_rows);
    return SF_ERR_ARG;
  }
  DeviceGuard guard(b->device);
  SF_FLUSH_VIEW(b, stream);
  return load_rows(b, lanes_dev, lane_idx64(idx_type), n, rows_dev, n_rows, row_idx_dev, obs_dev, (hipStream_t)stream);
}

extern "C" int sf_copy_lanes(sf_batch* dst, const void* dst_lanes_dev, sf_batch* src, const void* src_lanes_dev, int idx_type, int n,
                             void* obs_dev, void* stream) {
  int rc = lane_args(dst, dst_lanes_dev, idx_type, n, "sf_copy_lanes");
  if (rc == SF_OK) rc = lane_args(src, src_lanes_dev, idx_type, n, "sf_copy_lanes");
  if (rc == SF_OK) rc = lane_obs_ok(dst, obs_dev, "sf_copy_lanes");
  if (rc != SF_OK) return rc;
  uint32_t hd[4], hs[4];
  lane_header(dst, hd);
  lane_header(src, hs);
  if (memcmp(hd, hs, sizeof(hd)) != 0 || dst->device != src->device) {
    sf_set_error("sf_copy_lanes: the batches differ in preset, seed, spawn table or device (preset %u / %u, seed %u / %u, "
                 "table %u / %u, device %d / %d)", hd[1], hs[1], hd[2], hs[2], hd[3], hs[3], dst->device, src->device);
    return SF_ERR_ARG;
  }
  if (n == 0) return SF_OK;
  DeviceGuard guard(dst->device);
  hipStream_t st = (hipStream_t)stream;
  if (dst->lrows_cap < n) {  // scratch rows: made here, outside any capture
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(st, &cs));
    if (cs != hipStreamCaptureStatusNone) {
      sf_set_error("sf_copy_lanes: the batch's scratch holds %ld rows and %d are needed; make one eager call with that many "
                   "lanes before capturing", dst->lrows_cap, n);
      return SF_ERR_ARG;
    }
    HIP_TRY(hipStreamSynchronize(st));
    dst->d_lrows.reset();
    dst->lrows_cap = 0;
    HIP_TRY(dst->d_lrows.alloc((size_t)n * SF_LANE_STATE_BYTES));
    dst->lrows_cap = n;
  }
  SF_FLUSH_VIEW(src, st);
  SF_FLUSH_VIEW(dst, st);
  const int idx64 = lane_idx64(idx_type);
  // every source into the scratch rows first (a refused source lane leaves a row no batch takes), then the loads
  HIP_TRY(sf_launch_lanes_save(src->d_state.get(), src->n_envs, src_lanes_dev, idx64, n, dst->d_lrows.get(), hs, dst->d_lrefused, st));
  return load_rows(dst, dst_lanes_dev, idx64, n, dst->d_lrows.get(), n, nullptr, obs_dev, st);
}

extern "C" int sf_check_lanes(sf_batch* b, void* stream) {
  if (!b) return SF_ERR_ARG;
  DeviceGuard guard(b->device);
  unsigned long long bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, b->d_lrefused, sizeof(bad), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  if (bad) {
    HIP_TRY(hipMemsetAsync(b->d_lrefused, 0, sizeof(bad), (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    sf_set_error("%llu lane states were refused (lane or row index out of range, or a row from another preset / seed / spawn "
                 "table) and their lanes left as they were", bad);
    return SF_ERR_ARG;
  }
  return SF_OK;
}
