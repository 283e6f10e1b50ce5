// Exact 3-D Euclidean distance transform of mask volumes with integer voxel spacing for gfx950 (include/vdr.h:
// vdr_op_distance_transform_3d).  The squared distance (qz dz)^2 + (qy dy)^2 + (qx dx)^2 from a selected voxel to the nearest voxel
// that is not selected is an integer below 2^53 and a function of the mask and the spacing alone, so every output here is held bit
// for bit to rint(scipy.ndimage.distance_transform_edt(selected, sampling=(qz, qy, qx)) ^ 2).  The separable form, all integer:
//
//   edt3_row_kernel    edt.hip's row pass over the P Z planes of the call, through the SAME phase functions of edt_map.h: the signed
//                      16-bit row offset g along x goes to the workspace.
//   edt3_y_kernel      a thread per voxel, lanes along x: the in-plane vector (oy, ox), two int16, that attains
//                      min over y' of (qy (y - y'))^2 + (qx g(y', x))^2, by edt3_search_y, outwards from y' = y.  4 bytes a voxel
//                      instead of the 8 of the value; the value is recomputed from it (two multiplies) where it is read.
//   edt3_z_kernel      a thread per voxel, lanes along x: d2 = min over z' of (qz (z - z'))^2 + g2(vec(z', y, x)) by edt3_search_z,
//                      outwards from z' = z; slices are read through the cache, coalesced.  It writes d2 and the thresholded volume
//                      (each optional) and, for the peak, ONE partial slot per tile (plane_reduce.h's key reduction, twice: the
//                      largest d2, then the lowest index that attains it -- the pair does not fit one 64-bit key).
//   edt3_peak_kernel   one wave per volume reduces the volume's slots likewise.
//
// No atomics: every output and every slot has one writer (components.hip stays the only file with integer atomics).
// Every loop carries its termination argument beside it (here, in edt3d_map.h or in edt_map.h); the same code runs on the host
// first, thread by thread in both orders with every search under a step cap (tests/edt3d_map_cases.cpp).
// Built with -ffp-contract=off (Makefile) like its neighbours, although there is no floating point in it.
#include "vdr_dev.h"
#include "vdr_kernels.h"
#include "edt3d_map.h"
#include "plane_reduce.h"

namespace vdr {

namespace {

// blockIdx.y: the plane v Z + z
__global__ __launch_bounds__(EDT_THREADS) void edt3_row_kernel(const uint8_t* __restrict__ vol, EdtGeom q, int value, int outside_x,
                                                               short* __restrict__ g) {
  __shared__ short row[EDT_RROWS * EDT_ROW_LDS];
  __shared__ int sl[EDT_THREADS];
  __shared__ int sr[EDT_THREADS];
  const int tid = threadIdx.x, rb = blockIdx.x;
  const int64_t off = (int64_t)blockIdx.y * q.H * q.W;
  edt_row_load(q, rb, vol + off, value, tid, row);
  __syncthreads();
  edt_row_summary(q, rb, tid, row, sl, sr);
  __syncthreads();
  edt_row_scan(q, rb, outside_x, tid, row, sl, sr);
  __syncthreads();
  edt_row_store(q, rb, tid, row, g + off);
}

// blockIdx.x: the tile of the plane, blockIdx.y: the plane v Z + z
__global__ __launch_bounds__(EDT_THREADS) void edt3_y_kernel(const short* __restrict__ g, Edt3Geom q, long long thr, unsigned* __restrict__ vec) {
  const int tid = threadIdx.x, t = blockIdx.x;
  const int64_t off = (int64_t)blockIdx.y * q.H * q.W;
  const short* gp = g + off;
  for (int j = 0; j < EDT_CROWS; ++j) {  // fixed trip count; the search inside terminates (edt3_search_y)
    int y, x;
    edt_col_owner(q.pl, t, tid, j, &y, &x);
    if (x >= q.W || y >= q.H) continue;
    vec[off + y * q.W + x] = edt3_search_y(gp, q.H, q.W, y, x, q.qy, q.qx, (q.outside >> 1) & 1, thr).vec;
  }
}

// blockIdx.x: the tile of the plane, blockIdx.y: the slice z, blockIdx.z: the volume
__global__ __launch_bounds__(EDT_THREADS) void edt3_z_kernel(const unsigned* __restrict__ vec, Edt3Geom q, long long thr, long long r2,
                                                             long long* __restrict__ d2, uint8_t* __restrict__ within,
                                                             long long* __restrict__ slots) {
  __shared__ unsigned long long wred[EDT_RROWS];
  __shared__ unsigned long long wred2[EDT_RROWS];
  __shared__ unsigned long long top_s;
  const int tid = threadIdx.x, t = blockIdx.x, z = blockIdx.y, v = blockIdx.z;
  const int hw = q.H * q.W;
  const int64_t off = (int64_t)v * q.Z * hw;
  const unsigned* vp = vec + off;
  Edt3Peak pk = edt3_peak_none();
  for (int j = 0; j < EDT_CROWS; ++j) {  // fixed trip count; the search inside terminates (edt3_search_z)
    int y, x;
    edt_col_owner(q.pl, t, tid, j, &y, &x);
    if (x >= q.W || y >= q.H) continue;
    const int yx = y * q.W + x;
    const Edt3Hit h = edt3_search_z(vp, q.Z, hw, z, yx, q.qz, q.qy, q.qx, (q.outside >> 2) & 1, thr);
    const int i = z * hw + yx;
    if (d2) d2[off + i] = h.d2;
    if (within) within[off + i] = h.d2 <= r2 ? 1 : 0;
    edt3_peak_take(&pk, h.d2, i);
  }
  if (!slots) return;  // the same in every thread
  unsigned long long top = pr_block_max_key<EDT_THREADS / 64>((unsigned long long)pk.d2, wred);
  if (tid == 0) top_s = top;
  __syncthreads();
  top = top_s;
  const unsigned long long key = pr_block_max_key<EDT_THREADS / 64>(edt3_index_key(pk, (long long)top), wred2);
  if (tid == 0) {
    const int64_t s = edt3_slot(q, v, z, t);
    slots[s] = (long long)top, slots[s + 1] = edt3_index_of_key(key);
  }
}

// one wave per volume
__global__ __launch_bounds__(64) void edt3_peak_kernel(Edt3Geom q, const long long* __restrict__ slots, long long* __restrict__ peak) {
  const int v = blockIdx.x, lane = threadIdx.x;
  const long long* sp = slots + edt3_slot(q, v, 0, 0);
  Edt3Peak pk = edt3_peak_none();
  for (int t = lane; t < q.ztiles; t += 64) edt3_peak_take(&pk, sp[2 * (int64_t)t], sp[2 * (int64_t)t + 1]);  // ztiles is finite and t grows by 64
  const long long top = (long long)pr_wave_max_key((unsigned long long)pk.d2);  // in every lane
  const unsigned long long key = pr_wave_max_key(edt3_index_key(pk, top));
  if (lane == 0) peak[2 * v] = top, peak[2 * v + 1] = edt3_index_of_key(key);
}

}  // namespace

size_t distance_transform_3d_workspace_bytes(int P, int Z, int H, int W) {
  if (!edt3_shape_ok(P, Z, H, W)) return 0;
  return (size_t)edt3_work(P, Z, H, W).bytes;
}

// three launches, a fourth when the peak is asked for
hipError_t launch_distance_transform_3d(const uint8_t* vol, int P, int Z, int H, int W, int qz, int qy, int qx, int value, int outside,
                                        int64_t r2, void* work, int64_t* d2_out, int64_t* peak_out, uint8_t* within, hipStream_t s) {
  long long* d2 = reinterpret_cast<long long*>(d2_out);
  long long* peak = reinterpret_cast<long long*>(peak_out);
  if (!edt3_shape_ok(P, Z, H, W) || !edt3_spacing_ok(Z, H, W, qz, qy, qx) || (outside & ~7) || (!d2 && !peak && !within) || (within && r2 < 0))
    return hipErrorInvalidValue;
  const Edt3Geom q = edt3_geom(P, Z, H, W, qz, qy, qx, outside);
  const Edt3Work w = edt3_work(P, Z, H, W);
  short* g = (short*)((char*)work + w.g);
  unsigned* vec = (unsigned*)((char*)work + w.vec);
  long long* slots = peak ? (long long*)((char*)work + w.slots) : nullptr;
  const long long thr = within && !d2 && !peak ? r2 : -1;  // `within` alone: the searches may end early (edt3d_map.h)
  const unsigned planes = (unsigned)(P * Z);
  hipLaunchKernelGGL(edt3_row_kernel, dim3((unsigned)q.pl.rblocks, planes), dim3(EDT_THREADS), 0, s, vol, q.pl, value, outside & 1, g);
  hipLaunchKernelGGL(edt3_y_kernel, dim3((unsigned)q.pl.ctiles, planes), dim3(EDT_THREADS), 0, s, (const short*)g, q, thr, vec);
  hipLaunchKernelGGL(edt3_z_kernel, dim3((unsigned)q.pl.ctiles, (unsigned)Z, (unsigned)P), dim3(EDT_THREADS), 0, s, (const unsigned*)vec, q, thr, (long long)r2,
                     d2, within, slots);
  if (peak) hipLaunchKernelGGL(edt3_peak_kernel, dim3((unsigned)P), dim3(64), 0, s, q, (const long long*)slots, peak);
  return hipGetLastError();
}

}  // namespace vdr
