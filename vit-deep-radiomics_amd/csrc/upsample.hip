// Joint bilateral (guided) upsampling of dense descriptor maps for gfx950 (include/vdr.h: vdr_op_guide_lowres,
// vdr_op_upsample_guided).  Per output pixel a normalised weighted sum of the (2r+1)^2 low-resolution descriptors around its
// nearest patch; all pixels that share a nearest patch (a CELL of the image) share that window, so a cell is a small GEMM
// out[pixels, C] = W[pixels, window] . F[window, C] that contracts over the ROW index of the row-major descriptor map: the "tr"
// image of desc_tile.h.
//   up_lowres_kernel   one thread per (image, guide channel, patch): the mean of the guide over the patch's footprint into
//                      `work`; only the patches the box can reach are computed.
//   up_guided_kernel   256 threads; one work item = (image, cell that meets the box, chunk of 128 of the cell's pixels inside
//                      the box, group of UP_CTG 128-channel tiles).  Threads 0..127 build the weights of one pixel each -- hi and lo
//                      bf16 halves into two tr images [window slot][pixel], Z and the pixel's output offset into LDS -- ONCE; then
//                      per 128-channel tile the window's descriptor rows are staged through registers ([window slot][channel], slots
//                      outside the grid and past the window as zeros), ONE tr step of ceil((2r+1)^2 / 16) MFMA k-steps multiplies
//                      them, and the epilogue divides by Z and stores.  The slot of window position (a, b) is
//                      (a + r)(2r + 1) + (b + r) whatever the cell, so a pixel's bits do not depend on the tile it falls in, on the
//                      box or on the batch.
// No atomics; nothing but the low-resolution guide goes through `work`.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "desc_tile.h"
#include "vdr_dev.h"
#include "vdr_kernels.h"
#include "../../include/vdr.h"

namespace vdr {
namespace {

constexpr int UP_PIX = T128;                        // pixels of a chunk
constexpr int UP_CTG = 8;                           // 128-channel tiles per work item (the weights are built once per item)
// LDS of a radius: three tr images of the window's NKS * 16 slots (rows) each, Z [128] fp32, output offsets [128] int64 (-1: no
// pixel).  r = 1: 13.5 KB, r = 2: 25.5 KB, r = 3: 49.5 KB -- the workgroups per CU follow from it
constexpr int up_img(int r) { return ((2 * r + 1) * (2 * r + 1) + 15) / 16 * 16 * 256; }
constexpr int up_lds(int r) { return 3 * up_img(r) + 4 * UP_PIX + 8 * UP_PIX; }
static_assert(up_img(3) == TR_IMG && up_lds(3) <= 65536, "no opt-in to large dynamic LDS needed");

struct UpArgs {
  const void* f;
  int64_t ld, is;
  int C;
  const void* g;
  int g_bf16, Cg, H, W;
  float* glr;         // work: [batch][Cg][gh][gw] fp32
  const float* conf;  // [batch][gh][gw] or null
  int p, s, gh, gw;
  float cs, cr;
  int y0, x0, y1, x1;
  int ci0, cj0, nci, ncj, nchunks;  // the cells that meet the box; chunks of the largest of them
  int pi0, pj0, npi, npj;           // the patches those cells' windows reach
  int nct;
  void* out;
};

// first pixel row (column) whose nearest patch is i: the smallest Y with floor_div(2Y + 1 - p + s, 2s) >= i
__host__ __device__ inline int up_cell_lo(int i, int p, int s) { return i <= 0 ? 0 : (2 * s * i + p - s) / 2; }
__host__ __device__ inline int up_cell_hi(int i, int n, int p, int s, int size) { return i >= n - 1 ? size : up_cell_lo(i + 1, p, s); }

VDR_DEV float up_guide(const UpArgs& a, int64_t off) {
  return a.g_bf16 ? (float)((const bf16_t*)a.g)[off] : ((const float*)a.g)[off];
}

__global__ __launch_bounds__(256) void up_lowres_kernel(UpArgs a, int batch) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per = (int64_t)a.npi * a.npj;
  if (id >= per * a.Cg * batch) return;
  const int64_t bg = id / per;
  const int rem = (int)(id - bg * per);
  const int i = a.pi0 + rem / a.npj, j = a.pj0 + rem % a.npj;
  const int64_t base = (bg * a.H + (int64_t)i * a.s) * a.W + (int64_t)j * a.s;
  float sum = 0.0f;
  for (int ky = 0; ky < a.p; ++ky)
    for (int kx = 0; kx < a.p; ++kx) sum += up_guide(a, base + (int64_t)ky * a.W + kx);
  a.glr[(bg * a.gh + i) * a.gw + j] = __fdiv_rn(sum, (float)(a.p * a.p));
}

template <int R, bool FBF, bool OBF>
__global__ __launch_bounds__(256) void up_guided_kernel(UpArgs a) {
  constexpr int WIN = 2 * R + 1, NWIN = WIN * WIN, NKS = (NWIN + 15) / 16, QC = R * WIN + R, IMG = up_img(R);
  static_assert(IMG == NKS * 16 * 256, "an image holds the rows the k-steps read");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  int id = blockIdx.x;
  const int chunk = id % a.nchunks;
  id /= a.nchunks;
  const int cj = a.cj0 + id % a.ncj;
  id /= a.ncj;
  const int ci = a.ci0 + id % a.nci, b = id / a.nci;
  // the cell's pixels inside the box, row by row
  const int lo_y = up_cell_lo(ci, a.p, a.s), hi_y = up_cell_hi(ci, a.gh, a.p, a.s, a.H);
  const int lo_x = up_cell_lo(cj, a.p, a.s), hi_x = up_cell_hi(cj, a.gw, a.p, a.s, a.W);
  const int ys = lo_y > a.y0 ? lo_y : a.y0, ye = hi_y < a.y1 ? hi_y : a.y1;
  const int xs = lo_x > a.x0 ? lo_x : a.x0, xe = hi_x < a.x1 ? hi_x : a.x1;
  const int wx = xe - xs, npx = (ye - ys) * wx;
  const int first = chunk * UP_PIX;
  if (first >= npx) return;  // (uniform over the workgroup)
  const int ct0 = blockIdx.y * UP_CTG, ct1 = ct0 + UP_CTG < a.nct ? ct0 + UP_CTG : a.nct;

  char* s_hi = smem;
  char* s_lo = smem + IMG;
  char* s_f = smem + 2 * IMG;
  float* s_z = reinterpret_cast<float*>(smem + 3 * IMG);
  int64_t* s_off = reinterpret_cast<int64_t*>(smem + 3 * IMG + 4 * UP_PIX);

  // staging role: 16-byte chunk ch of the 128-channel tile, window slots rl, rl + 16, ... (one per MFMA k-step)
  const int ch = tid & 15, rl = tid >> 4;
  bool rok[NKS];
  int64_t roff[NKS];
#pragma unroll
  for (int j = 0; j < NKS; ++j) {
    const int slot = rl + 16 * j;
    const int pi = ci + slot / WIN - R, pj = cj + slot % WIN - R;
    rok[j] = slot < NWIN && pi >= 0 && pi < a.gh && pj >= 0 && pj < a.gw;
    roff[j] = rok[j] ? (int64_t)b * a.is + ((int64_t)pi * a.gw + pj) * a.ld : 0;
  }
  RawChunk<FBF> raw[NKS];
  // (a slot outside the grid or past the window and a channel past C are fetched as zeros and staged as zeros)
  const auto fetch = [&](int ct) {
    const int col = ct * 128 + ch * 8;
#pragma unroll
    for (int j = 0; j < NKS; ++j) raw_fill(raw[j], rok[j] && col < a.C, a.f, roff[j] + col);
  };
  const auto stage = [&]() {
#pragma unroll
    for (int j = 0; j < NKS; ++j) {
      bf16x8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (bf16_t)raw[j].get(e);
      *reinterpret_cast<bf16x8*>(s_f + tr_off(rl + 16 * j, ch)) = v;
    }
  };

  fetch(ct0);

  // ---- the weights of pixel tid of the chunk
  if (tid < UP_PIX) {
    const int t = first + tid;
    const bool ok = t < npx;
    const int Y = ok ? ys + t / wx : ys, X = ok ? xs + t % wx : xs;
    s_off[tid] = ok ? (((int64_t)b * (a.y1 - a.y0) + (Y - a.y0)) * (a.x1 - a.x0) + (X - a.x0)) * a.C : -1;
    float gp[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) gp[g] = g < a.Cg ? up_guide(a, (((int64_t)b * a.Cg + g) * a.H + Y) * a.W + X) : 0.0f;
    float z = 0.0f;
#pragma unroll
    for (int slot = 0; slot < NKS * 16; ++slot) {
      float w = 0.0f;
      if (slot < NWIN) {
        const int pi = ci + slot / WIN - R, pj = cj + slot % WIN - R;
        if (ok && pi >= 0 && pi < a.gh && pj >= 0 && pj < a.gw) {
          const float dy = (float)(2 * Y + 1 - a.p - 2 * a.s * pi) * 0.5f;
          const float dx = (float)(2 * X + 1 - a.p - 2 * a.s * pj) * 0.5f;
          const float ts = -(dy * dy + dx * dx) * a.cs;
          float dist2 = 0.0f;
#pragma unroll
          for (int g = 0; g < 4; ++g)
            if (g < a.Cg) {
              const float d = gp[g] - a.glr[(((int64_t)b * a.Cg + g) * a.gh + pi) * a.gw + pj];
              dist2 += d * d;
            }
          const float tr = -dist2 * a.cr;
          const float t2 = ts + tr;
          if (!(t2 < -64.0f)) {
            w = expf(t2);
            if (a.conf) w *= a.conf[((int64_t)b * a.gh + pi) * a.gw + pj];
          }
          z += w;
        }
      }
      const bf16_t h = (bf16_t)w;
      const bf16_t l = (bf16_t)(w - (float)h);
      const int off = tr_off(slot, tid >> 3) + 2 * (tid & 7);
      *reinterpret_cast<bf16_t*>(s_hi + off) = h;
      *reinterpret_cast<bf16_t*>(s_lo + off) = l;
    }
    s_z[tid] = z;
  }

  f32x16 acc[2][2];
  const tr_lds_cptr img_hi = (tr_lds_cptr)s_hi;
  const tr_lds_cptr img_lo = (tr_lds_cptr)s_lo;
  const tr_lds_cptr img_f = (tr_lds_cptr)s_f;
#pragma clang loop unroll(disable)
  for (int ct = ct0; ct < ct1; ++ct) {
    __syncthreads();  // every wave has read the previous tile
    stage();
    __syncthreads();
    if (ct + 1 < ct1) fetch(ct + 1);
    acc_zero(acc);
    tr_mfma_2a<NKS>(img_hi, img_lo, img_f, wr, wc, lane, acc);

    // ---- epilogue: a lane holds ONE channel per n and 16 pixels per m
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = acc_row(wr, m, e, hh);
        const int64_t off = s_off[row];
        const float z = s_z[row];
        if (off < 0) continue;
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const int tc = acc_col(wc, n, l31), col = ct * 128 + tc;
          if (col >= a.C) continue;
          float v;
          if (z == 0.0f) v = (float)*reinterpret_cast<const bf16_t*>(s_f + tr_off(QC, tc >> 3) + 2 * (tc & 7));  // the nearest patch
          else v = __fdiv_rn(acc[m][n][e], z);
          if (OBF) ((bf16_t*)a.out)[off + col] = (bf16_t)v;
          else ((float*)a.out)[off + col] = v;
        }
      }
  }
}

int up_nearest(int Y, int p, int s, int n) {
  const int num = 2 * Y + 1 - p + s, den = 2 * s;
  int q = num / den;
  if (num % den < 0) --q;
  return q < 0 ? 0 : q > n - 1 ? n - 1 : q;
}

// the launch geometry of a box: cells, chunks and the patch range of the low-resolution guide
void up_geometry(UpArgs& a, int r) {
  a.ci0 = up_nearest(a.y0, a.p, a.s, a.gh);
  a.cj0 = up_nearest(a.x0, a.p, a.s, a.gw);
  const int ci1 = up_nearest(a.y1 - 1, a.p, a.s, a.gh), cj1 = up_nearest(a.x1 - 1, a.p, a.s, a.gw);
  a.nci = ci1 - a.ci0 + 1;
  a.ncj = cj1 - a.cj0 + 1;
  int mh = 0, mw = 0;
  for (int i = a.ci0; i <= ci1; ++i) {
    const int lo = up_cell_lo(i, a.p, a.s), hi = up_cell_hi(i, a.gh, a.p, a.s, a.H);
    const int h = (hi < a.y1 ? hi : a.y1) - (lo > a.y0 ? lo : a.y0);
    mh = h > mh ? h : mh;
  }
  for (int j = a.cj0; j <= cj1; ++j) {
    const int lo = up_cell_lo(j, a.p, a.s), hi = up_cell_hi(j, a.gw, a.p, a.s, a.W);
    const int w = (hi < a.x1 ? hi : a.x1) - (lo > a.x0 ? lo : a.x0);
    mw = w > mw ? w : mw;
  }
  a.nchunks = (int)(((int64_t)mh * mw + UP_PIX - 1) / UP_PIX);
  a.pi0 = a.ci0 - r > 0 ? a.ci0 - r : 0;
  a.pj0 = a.cj0 - r > 0 ? a.cj0 - r : 0;
  a.npi = (ci1 + r < a.gh - 1 ? ci1 + r : a.gh - 1) - a.pi0 + 1;
  a.npj = (cj1 + r < a.gw - 1 ? cj1 + r : a.gw - 1) - a.pj0 + 1;
}

hipError_t up_lowres(const UpArgs& a, int batch, hipStream_t st) {
  const int64_t n = (int64_t)a.npi * a.npj * a.Cg * batch;
  if ((n + 255) / 256 > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(up_lowres_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, batch);
  return hipGetLastError();
}

template <int R>
hipError_t up_launch(const UpArgs& a, bool fbf, bool obf, dim3 grid, hipStream_t st) {
  if (fbf && obf) hipLaunchKernelGGL((up_guided_kernel<R, true, true>), grid, dim3(256), up_lds(R), st, a);
  else if (fbf) hipLaunchKernelGGL((up_guided_kernel<R, true, false>), grid, dim3(256), up_lds(R), st, a);
  else if (obf) hipLaunchKernelGGL((up_guided_kernel<R, false, true>), grid, dim3(256), up_lds(R), st, a);
  else hipLaunchKernelGGL((up_guided_kernel<R, false, false>), grid, dim3(256), up_lds(R), st, a);
  return hipGetLastError();
}

}  // namespace

size_t upsample_work_bytes(int batch, int Cg, int gh, int gw) {
  if (batch <= 0 || Cg <= 0 || gh <= 0 || gw <= 0) return 0;
  const int64_t n = (int64_t)batch * Cg * gh * gw;
  return (size_t)(((n + 3) & ~(int64_t)3) * 4);
}

hipError_t launch_guide_lowres(const void* guide, bool guide_bf16, int batch, int Cg, int H, int W, int p, int s, int gh, int gw,
                               float* work, hipStream_t st) {
  if (!guide || !work) return hipErrorInvalidValue;
  UpArgs a = {};
  a.g = guide, a.g_bf16 = guide_bf16, a.Cg = Cg, a.H = H, a.W = W, a.glr = work;
  a.p = p, a.s = s, a.gh = gh, a.gw = gw;
  a.pi0 = a.pj0 = 0, a.npi = gh, a.npj = gw;
  return up_lowres(a, batch, st);
}

hipError_t launch_upsample_guided(const void* f, bool f_bf16, int64_t ld, int64_t image_stride, int batch, int gh, int gw, int C,
                                  const void* guide, bool guide_bf16, int Cg, int H, int W, int p, int s, int radius, float cs,
                                  float cr, const float* conf, int y0, int x0, int y1, int x1, float* work, void* out, bool out_bf16,
                                  hipStream_t st) {
  if (!f || !guide || !work || !out || radius < 1 || radius > 3 || Cg < 1 || Cg > 4 || C <= 0 || (C & 7) || ld < C || batch <= 0 ||
      s <= 0 || p % s || gh <= 0 || gw <= 0 || H != p + (gh - 1) * s || W != p + (gw - 1) * s || y0 < 0 || x0 < 0 || y1 > H ||
      x1 > W || y0 >= y1 || x0 >= x1)
    return hipErrorInvalidValue;
  UpArgs a = {};
  a.f = f, a.ld = ld, a.is = image_stride, a.C = C;
  a.g = guide, a.g_bf16 = guide_bf16, a.Cg = Cg, a.H = H, a.W = W, a.glr = work, a.conf = conf;
  a.p = p, a.s = s, a.gh = gh, a.gw = gw, a.cs = cs, a.cr = cr;
  a.y0 = y0, a.x0 = x0, a.y1 = y1, a.x1 = x1;
  a.nct = (C + 127) / 128;
  a.out = out;
  up_geometry(a, radius);
  const int64_t items = (int64_t)batch * a.nci * a.ncj * a.nchunks;
  const int groups = (a.nct + UP_CTG - 1) / UP_CTG;
  if (items > INT32_MAX || groups > 65535) return hipErrorInvalidValue;
  if (hipError_t e = up_lowres(a, batch, st)) return e;
  const dim3 grid((unsigned)items, (unsigned)groups);
  return radius == 1 ? up_launch<1>(a, f_bf16, out_bf16, grid, st)
         : radius == 2 ? up_launch<2>(a, f_bf16, out_bf16, grid, st)
                       : up_launch<3>(a, f_bf16, out_bf16, grid, st);
}

}  // namespace vdr
