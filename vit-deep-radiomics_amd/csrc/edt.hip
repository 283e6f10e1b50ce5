// Exact Euclidean distance transform of mask planes for gfx950 (include/vdr.h: vdr_op_distance_transform).  The squared distance
// from a selected pixel to the nearest pixel that is not selected is an integer and a function of the mask alone, so every output
// here is held bit for bit to scipy.ndimage.distance_transform_edt.  The separable form, all integer:
//
//   edt_row_kernel     a workgroup owns four rows of one plane, a wave a row (edt_map.h): the row goes to LDS, every lane takes
//                      the last and first non-selected column of its own segment, then walks the segment forwards and backwards
//                      from its neighbours' summaries; the ROW OFFSET g (int16, signed: towards the nearest non-selected pixel of
//                      the row, the lower column on a tie) goes to the workspace, lane-contiguous.
//   edt_col_kernel     a thread per pixel, lanes along x: d2 = min over y' of (y - y')^2 + g(y', x)^2 by edt_search, outwards from
//                      y' = y until k^2 reaches the best so far; g rows are read through the cache, coalesced.  It writes d2,
//                      nearest, the thresholded plane (each optional) and, for the peak, ONE partial slot per tile: the
//                      largest key of the workgroup (edt_peak_key; the key reduction of plane_reduce.h).
//   edt_peak_kernel    one wave per plane reduces the plane's slots to (largest d2, lowest index that attains it), likewise.
//
// No atomics: every output and every slot has one writer (components.hip stays the only file with integer atomics).
// Every loop carries its termination argument beside it (here or in edt_map.h); the same code runs on the host first, thread by
// thread in both orders with every search under a step cap (tests/edt_map_cases.cpp).
// Built with -ffp-contract=off (Makefile) like its neighbours, although there is no floating point in it.
#include "vdr_dev.h"
#include "vdr_kernels.h"
#include "edt_map.h"
#include "plane_reduce.h"

namespace vdr {

namespace {

__global__ __launch_bounds__(EDT_THREADS) void edt_row_kernel(const uint8_t* __restrict__ mask, EdtGeom q, int value, int outside,
                                                              short* __restrict__ g) {
  __shared__ short row[EDT_RROWS * EDT_ROW_LDS];
  __shared__ int sl[EDT_THREADS];
  __shared__ int sr[EDT_THREADS];
  const int tid = threadIdx.x, rb = blockIdx.x;
  const int64_t off = (int64_t)blockIdx.y * q.H * q.W;
  edt_row_load(q, rb, mask + off, value, tid, row);
  __syncthreads();
  edt_row_summary(q, rb, tid, row, sl, sr);
  __syncthreads();
  edt_row_scan(q, rb, outside, tid, row, sl, sr);
  __syncthreads();
  edt_row_store(q, rb, tid, row, g + off);
}

__global__ __launch_bounds__(EDT_THREADS) void edt_col_kernel(const short* __restrict__ g, EdtGeom q, int outside, int r2,
                                                              int32_t* __restrict__ d2, int32_t* __restrict__ nearest,
                                                              uint8_t* __restrict__ within, int32_t* __restrict__ slots) {
  __shared__ unsigned long long wred[EDT_RROWS];
  const int tid = threadIdx.x, t = blockIdx.x, plane = blockIdx.y;
  const int64_t off = (int64_t)plane * q.H * q.W;
  const short* gp = g + off;
  unsigned long long key = 0;
  for (int j = 0; j < EDT_CROWS; ++j) {  // fixed trip count; the search inside terminates (edt_search)
    int y, x;
    edt_col_owner(q, t, tid, j, &y, &x);
    if (x >= q.W || y >= q.H) continue;
    const EdtHit h = edt_search(gp, q.H, q.W, y, x, outside, nearest != nullptr);
    const int i = y * q.W + x;
    if (d2) d2[off + i] = h.d2;
    if (nearest) nearest[off + i] = h.yn < 0 ? -1 : h.yn * q.W + x + gp[h.yn * q.W + x];
    if (within) within[off + i] = h.d2 <= r2 ? 1 : 0;
    const unsigned long long u = edt_peak_key(h.d2, i);
    key = u > key ? u : key;
  }
  if (!slots) return;  // the same in every thread
  key = pr_block_max_key<EDT_THREADS / 64>(key, wred);
  if (tid == 0) {
    const int64_t s = edt_slot(q, plane, t);
    slots[s] = edt_peak_d2(key), slots[s + 1] = edt_peak_index(key);
  }
}

// one wave per plane
__global__ __launch_bounds__(64) void edt_peak_kernel(EdtGeom q, const int32_t* __restrict__ slots, int32_t* __restrict__ peak) {
  const int plane = blockIdx.x, lane = threadIdx.x;
  unsigned long long key = 0;
  for (int t = lane; t < q.ctiles; t += 64) {  // ctiles is finite and t grows by 64
    const int64_t s = edt_slot(q, plane, t);
    const unsigned long long u = slots[s + 1] < 0 ? 0ull : edt_peak_key(slots[s], slots[s + 1]);
    key = u > key ? u : key;
  }
  key = pr_wave_max_key(key);
  if (lane == 0) peak[2 * plane] = edt_peak_d2(key), peak[2 * plane + 1] = edt_peak_index(key);
}

bool edt_shape_ok(int P, int H, int W) { return P >= 1 && P <= EDT_MAX_PLANES && H >= 1 && H <= EDT_MAX_SIDE && W >= 1 && W <= EDT_MAX_SIDE; }

}  // namespace

size_t distance_transform_workspace_bytes(int P, int H, int W) {
  if (!edt_shape_ok(P, H, W)) return 0;
  return (size_t)edt_work(edt_geom(P, H, W)).bytes;
}

// two launches, a third when the peak is asked for
hipError_t launch_distance_transform(const uint8_t* mask, int P, int H, int W, int value, int outside, int r2, void* work, int32_t* d2,
                                     int32_t* nearest, int32_t* peak, uint8_t* within, hipStream_t s) {
  if (!edt_shape_ok(P, H, W) || (nearest && outside) || (!d2 && !nearest && !peak && !within) || (within && r2 < 0)) return hipErrorInvalidValue;
  const EdtGeom q = edt_geom(P, H, W);
  const EdtWork w = edt_work(q);
  short* g = (short*)((char*)work + w.g);
  int32_t* slots = peak ? (int32_t*)((char*)work + w.slots) : nullptr;
  hipLaunchKernelGGL(edt_row_kernel, dim3((unsigned)q.rblocks, (unsigned)P), dim3(EDT_THREADS), 0, s, mask, q, value, outside, g);
  hipLaunchKernelGGL(edt_col_kernel, dim3((unsigned)q.ctiles, (unsigned)P), dim3(EDT_THREADS), 0, s, (const short*)g, q, outside, r2, d2, nearest,
                     within, slots);
  if (peak) hipLaunchKernelGGL(edt_peak_kernel, dim3((unsigned)P), dim3(64), 0, s, q, (const int32_t*)slots, peak);
  return hipGetLastError();
}

}  // namespace vdr
