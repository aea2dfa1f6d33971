// sf_episode_log.hip -- the episode log (include/sfmi.h: sf_eplog_*): one record per finished episode in a ring, and a
// histogram of episode returns, kept on the device from the (reward, done, info, action) rows of every step -- what the
// trainer's log line (rl/train.py:158-165: mean / median / min / max) and the evaluator's per-episode line
// (rl/evaluate.py:82-99: return, fortresses destroyed, shots) are made of.
//
// Game over is time-only, so the envs of a fresh batch all finish on one tick: a whole batch appends at once.  The order of
// the ring is therefore COMPUTED, never raced for: record (k, e) of an update gets sequence number total + the number of
// set bytes of `done` in front of it in row-major order.  Reduce-then-scan, three launches per group of SF_EPLOG_ROWS rows:
//
//   sf_eplog_count_kernel   one workgroup per cell = (row, tile of 256 envs): the set `done` bytes of the cell (ballot,
//                           popcount, four wave counts through LDS).
//   sf_eplog_scan_kernel    ONE workgroup: exclusive prefix sum over the cells in row-major order (256 cells per pass, a
//                           carry between passes); then lane 0 publishes base_seq = total, base_row = rows_seen and advances
//                           total and rows_seen -- the counters live on the device, so a replayed graph goes on counting.
//   sf_eplog_apply_kernel   one thread per env, the four accumulators in registers over the group's rows.  Only in a cell
//                           whose count is not zero (uniform across the workgroup: the count is a scalar load) is `done`
//                           read at all; there a lane ranks itself among the cell's ends by ballot + mbcnt and the
//                           prefix of the waves in front of it (LDS, one barrier), and stores its record to slot
//                           seq % capacity with plain stores -- unless the update overflows the ring and a later record of
//                           the same launch owns that slot (seq + capacity < total afterwards): no two lanes store to
//                           one slot.  Histogram adds are integer global atomics (commutative: the bins do not depend on
//                           their order); ends are rare -- one per env and game -- so they are not staged in LDS.
//
// No workgroup waits for another; nothing is ordered by an atomic.  Rows beyond SF_EPLOG_ROWS go through the same three
// launches again, which is the same as a second update: sequence numbers are row-major either way.
#include <hip/hip_runtime.h>

#include "sf_internal.h"

namespace {

constexpr int kTile = 256;

__global__ __launch_bounds__(256) void sf_eplog_count_kernel(const uint8_t* __restrict__ done, int n, int tiles,
                                                             uint32_t* __restrict__ counts) {
  __shared__ uint32_t wsum[4];
  const int cell = blockIdx.x;  // row * tiles + tile
  const int k = cell / tiles, t = cell - k * tiles;
  const int e = t * kTile + (int)threadIdx.x;
  const bool d = e < n && done[(int64_t)k * n + e] != 0;
  const unsigned long long m = __ballot(d);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) counts[cell] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(256) void sf_eplog_scan_kernel(const uint32_t* __restrict__ counts, uint32_t* __restrict__ offs,
                                                            int cells, int rows, SfEplogHeader* __restrict__ h) {
  __shared__ uint32_t wtot[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (int base = 0; base < cells; base += 256) {  // (uniform trip count)
    const int i = base + (int)threadIdx.x;
    const uint32_t v = i < cells ? counts[i] : 0u;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t u = __shfl_up(inc, d, 64);
      if (lane >= d) inc += u;
    }
    if (lane == 63) wtot[w] = inc;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t x = wtot[j];
      pre += j < w ? x : 0u;
      tot += x;
    }
    if (i < cells) offs[i] = carry + pre + inc - v;
    carry += tot;
    __syncthreads();  // (wtot is written again in the next pass)
  }
  if (threadIdx.x == 0) {
    const unsigned long long total = h->total, seen = h->rows_seen;
    h->base_seq = total;
    h->base_row = seen;
    h->total = total + carry;
    h->rows_seen = seen + (unsigned long long)rows;
  }
}

template <typename A>
__global__ __launch_bounds__(256) void sf_eplog_apply_kernel(SfEplogArgs a, const int32_t* __restrict__ rew,
                                                             const uint8_t* __restrict__ done, const uint8_t* __restrict__ info,
                                                             const A* __restrict__ act, int rows, int tiles) {
  __shared__ uint32_t wcnt[2][4];
  const int tile = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int e = tile * kTile + (int)threadIdx.x;
  const bool live = e < a.n;
  int4 acc = make_int4(0, 0, 0, 0);  // ret, length, kills, fire
  if (live) acc = a.acc[e];
  const unsigned long long base = a.hdr->base_seq, total = a.hdr->total;  // (total: after this group of rows)
  const long long row0 = (long long)a.hdr->base_row;
  int phase = 0;
  for (int k = 0; k < rows; k++) {
    const int64_t i = (int64_t)k * a.n + e;
    if (live) {
      acc.x += rew[i];
      acc.y += 1;
      acc.z += info[i];
      if (act) acc.w += ((long long)act[i] == (long long)a.fire_action) ? 1 : 0;
    }
    const int cell = k * tiles + tile;
    if (a.counts[cell] == 0u) continue;  // (uniform across the workgroup: nobody of this tile finished on this row)
    const bool d = live && done[i] != 0;
    const unsigned long long m = __ballot(d);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (lane == 0) wcnt[phase][w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t pre = 0;
#pragma unroll
    for (int j = 0; j < 3; j++) pre += j < w ? wcnt[phase][j] : 0u;
    phase ^= 1;  // (the next barrier lies between these reads and the next writes of this half)
    if (d) {
      const unsigned long long seq = base + a.offs[cell] + pre + rank;
      if (seq + a.capacity >= total) {  // else a later record of this launch owns the slot
        sf_episode_record r;
        r.env = e;
        r.episode_return = acc.x;
        r.length = acc.y;
        r.kills = acc.z;
        r.fire_actions = acc.w;
        r.reserved = 0;
        r.end_row = row0 + k;
        a.ring[seq % a.capacity] = r;
      }
      long long bin = (long long)acc.x - a.hist_lo;
      bin = bin < 0 ? 0 : (bin > a.bins - 1 ? a.bins - 1 : bin);
      atomicAdd(a.hist + bin, 1ull);
      acc = make_int4(0, 0, 0, 0);
    }
  }
  if (live) a.acc[e] = acc;
}

// sf_eplog_restart_where: the marked envs' running accumulators start over; nothing else of the log is touched
__global__ __launch_bounds__(256) void sf_eplog_restart_where_kernel(int4* __restrict__ acc, const uint8_t* __restrict__ mask, int n) {
  const int e = blockIdx.x * kTile + (int)threadIdx.x;
  if (e < n && mask[e] != 0) acc[e] = make_int4(0, 0, 0, 0);
}

}  // namespace

hipError_t sf_launch_eplog_restart_where(const SfEplogArgs& a, const uint8_t* mask, hipStream_t stream) {
  hipLaunchKernelGGL(sf_eplog_restart_where_kernel, dim3((unsigned)((a.n + kTile - 1) / kTile)), dim3(256), 0, stream, a.acc, mask, a.n);
  return hipGetLastError();
}

hipError_t sf_launch_eplog_update(const SfEplogArgs& a, const int32_t* rew, const uint8_t* done, const uint8_t* info,
                                  const void* actions, int act_type, int K, hipStream_t stream) {
  const int tiles = (a.n + kTile - 1) / kTile;
  const size_t act_size = act_type == SF_ACT_I64 ? 8 : act_type == SF_ACT_I32 ? 4 : 1;
  for (int k0 = 0; k0 < K; k0 += SF_EPLOG_ROWS) {
    const int rows = K - k0 < SF_EPLOG_ROWS ? K - k0 : SF_EPLOG_ROWS;
    const size_t at = (size_t)k0 * (size_t)a.n;
    const void* act = actions ? (const void*)((const unsigned char*)actions + at * act_size) : nullptr;
    hipLaunchKernelGGL(sf_eplog_count_kernel, dim3((unsigned)(rows * tiles)), dim3(256), 0, stream, done + at, a.n, tiles, a.counts);
    hipLaunchKernelGGL(sf_eplog_scan_kernel, dim3(1), dim3(256), 0, stream, a.counts, a.offs, rows * tiles, rows, a.hdr);
    const dim3 grid((unsigned)tiles), block(256);
    if (act_type == SF_ACT_I64)
      hipLaunchKernelGGL(sf_eplog_apply_kernel<int64_t>, grid, block, 0, stream, a, rew + at, done + at, info + at, (const int64_t*)act, rows, tiles);
    else if (act_type == SF_ACT_I32)
      hipLaunchKernelGGL(sf_eplog_apply_kernel<int32_t>, grid, block, 0, stream, a, rew + at, done + at, info + at, (const int32_t*)act, rows, tiles);
    else
      hipLaunchKernelGGL(sf_eplog_apply_kernel<uint8_t>, grid, block, 0, stream, a, rew + at, done + at, info + at, (const uint8_t*)act, rows, tiles);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}
