// The prompt side of SAM's mask decoder beyond boxes, for gfx950 (include/vdr.h, "mask prompt ops"):
//
//   mask_embed      the keys of a decode with a dense mask prompt in ONE pass: per cell the 4 x 4 mask pixels go through
//                   mask_downscaling (conv 1->4 k2 s2, LayerNorm2d, GELU, conv 4->16 k2 s2, LayerNorm2d, GELU, conv 16->256 k1),
//                   the image embedding is added and the sum is rounded once to bf16.  `dense` is never written.  A workgroup
//                   owns ME_CELLS consecutive rows of keys (mask_embed_map.h): the embedding tile is staged in LDS (16-byte
//                   chunks for the channel-last layout; for the channel-first one lanes run along the cells, so neither the
//                   read nor the LDS write is strided by n), thread c holds conv3's 16 weights of channel c in registers and
//                   walks the tile's cells, the bf16 tile leaves through LDS in 16-byte chunks (the rows of a tile are one
//                   contiguous run of keys).
//   prompt_tokens   decoder_tokens_kernel's sibling for segment_anything's layout [iou; 4 mask tokens; np points; one padding
//                   point if there is no box; 2 box corners if there is one].  Trigonometry in double, once per decode; with
//                   boxes only it computes decoder_tokens_kernel's bits.
//   mask_box        the box of a logit map (> threshold) for the next slice of a volume: one workgroup per problem, a count
//                   and a box by the plane reduction of plane_reduce.h, no atomics.
//
// Built with -ffp-contract=off (Makefile): every multiply and add outside the explicit fmaf calls is rounded once.
#include "vdr_dev.h"
#include "vdr_kernels.h"
#include "mask_embed_map.h"
#include "plane_reduce.h"

namespace vdr {

namespace {

// ---- mask_embed ------------------------------------------------------------------------------------------------------------
constexpr int ME_LD = 258;  // fp32 row of the staged embedding tile: 2 mod 64, so the 32 cells x 2 channels a wave writes in the
                            // channel-first staging fall into 64 different banks
// the small weights, one fp32 buffer (vdr_api.hip packs it): offsets
constexpr int ME_W1 = 0, ME_B1 = 16, ME_G1 = 20, ME_E1 = 24, ME_W2 = 28, ME_B2 = 284, ME_G2 = 300, ME_E2 = 316;
static_assert(ME_E2 + 16 == MASK_EMBED_SMALL, "the packed small weights");

__global__ __launch_bounds__(256) void mask_embed_kernel(const float* __restrict__ emb, const float* __restrict__ mask,
                                                         const float* __restrict__ small, const float* __restrict__ w3g,
                                                         const float* __restrict__ b3g, bf16_t* __restrict__ keys, MeGeom q, float eps) {
  __shared__ float E[ME_CELLS * ME_LD];
  __shared__ __attribute__((aligned(16))) bf16_t O[ME_CELLS * ME_C];
  __shared__ __attribute__((aligned(16))) float pix[ME_CELLS * 16];
  __shared__ __attribute__((aligned(16))) float a1[ME_CELLS * 16];
  __shared__ __attribute__((aligned(16))) float c2[ME_CELLS * 16];
  __shared__ __attribute__((aligned(16))) float a2[ME_CELLS * 16];
  __shared__ float sw[MASK_EMBED_SMALL];
  const int tid = threadIdx.x;
  const long long tile = blockIdx.x;
  for (int i = tid; i < MASK_EMBED_SMALL; i += 256) sw[i] = small[i];
  float w3[16];
#pragma unroll
  for (int k4 = 0; k4 < 4; ++k4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(w3g + tid * 16 + 4 * k4);
#pragma unroll
    for (int e = 0; e < 4; ++e) w3[4 * k4 + e] = t[e];
  }
  const float b3 = b3g[tid];
  if (q.channels_last) {
    for (int idx = tid; idx < ME_CELLS * (ME_C / 4); idx += 256) {
      const int k = idx & (ME_C / 4 - 1), i = idx / (ME_C / 4);
      const MeRow r = me_row(q, tile, i);
      const f32x4 v = *reinterpret_cast<const f32x4*>(emb + me_emb_offset(q, r, 4 * k));
#pragma unroll
      for (int e = 0; e < 4; ++e) E[i * ME_LD + 4 * k + e] = v[e];
    }
  } else {
    for (int idx = tid; idx < ME_CELLS * ME_C; idx += 256) {
      const int i = idx & (ME_CELLS - 1), c = idx / ME_CELLS;
      const MeRow r = me_row(q, tile, i);
      E[i * ME_LD + c] = emb[me_emb_offset(q, r, c)];
    }
  }
  const int i = tid >> 2, sub = tid & 3;  // (tid < 128: cell i of the tile, quarter sub)
  if (tid < 4 * ME_CELLS) {
    const MeRow r = me_row(q, tile, i);
    *reinterpret_cast<f32x4*>(pix + i * 16 + 4 * sub) = *reinterpret_cast<const f32x4*>(mask + me_mask_offset(q, r, sub));
  }
  __syncthreads();
  if (tid < 4 * ME_CELLS) {  // conv1 on the 2 x 2 block (by, bx) = (sub >> 1, sub & 1), LayerNorm over its 4 channels, GELU
    const int by = sub >> 1, bx = sub & 1;
    const float* px = pix + i * 16 + 8 * by + 2 * bx;
    const float x[4] = {px[0], px[1], px[4], px[5]};
    float c[4];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      float acc = sw[ME_B1 + ch];
#pragma unroll
      for (int k = 0; k < 4; ++k) acc = fmaf(sw[ME_W1 + 4 * ch + k], x[k], acc);
      c[ch] = acc;
    }
    const float mean = (((c[0] + c[1]) + c[2]) + c[3]) / 4.0f;
    float d[4], ss = 0.0f;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      d[ch] = c[ch] - mean;
      ss = ss + d[ch] * d[ch];
    }
    const float rstd = 1.0f / sqrtf(ss / 4.0f + eps);
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) a1[i * 16 + 4 * ch + sub] = gelu_erf((d[ch] * rstd) * sw[ME_G1 + ch] + sw[ME_E1 + ch]);
  }
  __syncthreads();
  if (tid < 4 * ME_CELLS) {  // conv2: 4 of the 16 output channels per thread, 16 inputs (ci * 4 + dy * 2 + dx)
    float h[16];
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(a1 + i * 16 + 4 * k4);
#pragma unroll
      for (int e = 0; e < 4; ++e) h[4 * k4 + e] = t[e];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = 4 * sub + j;
      float acc = sw[ME_B2 + co];
#pragma unroll
      for (int k = 0; k < 16; ++k) acc = fmaf(sw[ME_W2 + 16 * co + k], h[k], acc);
      c2[i * 16 + co] = acc;
    }
  }
  __syncthreads();
  if (tid < 4 * ME_CELLS) {  // LayerNorm over the 16 channels (each of the cell's 4 threads sums them in the same order), GELU
    float c[16], s = 0.0f;
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(c2 + i * 16 + 4 * k4);
#pragma unroll
      for (int e = 0; e < 4; ++e) c[4 * k4 + e] = t[e];
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) s = s + c[k];
    const float mean = s / 16.0f;
    float ss = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float d = c[k] - mean;
      ss = ss + d * d;
    }
    const float rstd = 1.0f / sqrtf(ss / 16.0f + eps);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = 4 * sub + j;
      a2[i * 16 + co] = gelu_erf(((c[co] - mean) * rstd) * sw[ME_G2 + co] + sw[ME_E2 + co]);
    }
  }
  __syncthreads();
  for (int r = 0; r < ME_CELLS; ++r) {  // conv3: channel tid of every cell of the tile
    float acc = b3;
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(a2 + r * 16 + 4 * k4);  // (one address for the wave: an LDS broadcast)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = fmaf(w3[4 * k4 + e], t[e], acc);
    }
    O[r * ME_C + tid] = (bf16_t)(acc + E[r * ME_LD + tid]);
  }
  __syncthreads();
  const long long row0 = tile * ME_CELLS;
  const long long left = q.rows - row0;
  const int chunks = (int)(left < ME_CELLS ? left : ME_CELLS) * (ME_C / 8);
  for (int idx = tid; idx < chunks; idx += 256)
    *reinterpret_cast<bf16x8*>(keys + row0 * ME_C + 8 * idx) = *reinterpret_cast<const bf16x8*>(O + 8 * idx);
}

// ---- prompt tokens -----------------------------------------------------------------------------------------------------------
struct PromptTokArgs {
  const float* boxes;
  const float* points;
  const int32_t* labels;
  const float* fixed;
  const float* gauss;
  const float* corner;
  const float* pt_emb;  // [2, 256]: point_embeddings[0] (background), [1] (foreground)
  const float* nap;     // [256]: not_a_point_embed
  bf16_t* tok;
  int P, np, T;
  float img;
};

__device__ double fourier_phase(double px, double py, double img, const float* gauss, int f) {
  const double x = (px + 0.5) / img, y = (py + 0.5) / img;
  return 6.283185307179586476925286766559 * ((2.0 * x - 1.0) * (double)gauss[f] + (2.0 * y - 1.0) * (double)gauss[128 + f]);
}

__global__ void prompt_tokens_kernel(PromptTokArgs a) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.P * a.T * 256) return;
  const int c = idx & 255, t = (idx >> 8) % a.T, p = idx / (a.T * 256);
  const int f = c & 127;
  float v;
  if (t < 5) {
    v = a.fixed[t * 256 + c];
  } else if (t < 5 + a.np) {
    const int j = p * a.np + (t - 5);
    const int label = a.labels[j];
    if (label == -1) {
      v = a.nap[c];
    } else if (label == -10) {
      v = 0.0f;
    } else {
      const double ph = fourier_phase((double)a.points[2 * j], (double)a.points[2 * j + 1], (double)a.img, a.gauss, f);
      double e = c < 128 ? sin(ph) : cos(ph);
      if (label == 0 || label == 1) e = e + (double)a.pt_emb[label * 256 + c];
      v = (float)e;
    }
  } else if (a.boxes) {
    const int corner_i = t - 5 - a.np;
    const double ph = fourier_phase((double)a.boxes[p * 4 + 2 * corner_i], (double)a.boxes[p * 4 + 2 * corner_i + 1], (double)a.img, a.gauss, f);
    v = (float)((c < 128 ? sin(ph) : cos(ph)) + (double)a.corner[corner_i * 256 + c]);
  } else {
    v = a.nap[c];  // the padding point: a label -1 row
  }
  a.tok[idx] = (bf16_t)v;
}

// ---- mask_box ----------------------------------------------------------------------------------------------------------------
// VEC: W % 4 == 0 and every plane 16-byte aligned -- a lane reads 4 pixels of one row per load (the sweep's 256 x 256 plane is 64
// loads a lane instead of 256; the kernel is latency-bound at one workgroup per problem)
template <bool VEC>
__global__ __launch_bounds__(256) void mask_box_kernel(const float* __restrict__ logits, int64_t plane_stride, const float* __restrict__ prev,
                                                       float* __restrict__ boxes, int32_t* __restrict__ area, int H, int W, float img,
                                                       float margin, float threshold) {
  __shared__ int wred[4][PR_SLOT];
  const int p = blockIdx.x, tid = threadIdx.x;
  const float* lg = logits + (int64_t)p * plane_stride;
  PlaneAcc<1> acc = pr_identity<1>(W, H);  // the one sum: the count
  const int total = H * W;
  auto take = [&](int x, int y) {
    acc.take(x, y);
    ++acc.sum(0);
  };
  if (VEC) {
    for (int idx = 4 * tid; idx < total; idx += 4 * 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(lg + idx);
      const int y = idx / W, x = idx - y * W;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (v[e] > threshold) take(x + e, y);
    }
  } else {
    for (int idx = tid; idx < total; idx += 256) {
      if (lg[idx] > threshold) {
        const int y = idx / W;
        take(idx - y * W, y);
      }
    }
  }
  pr_block_reduce<1, 4>(acc, wred);
  if (tid >= 4) return;
  const int n = pr_waves_value<1, 4>(wred, 0);
  if (tid == 0) area[p] = n;
  float v;
  if (n == 0) {
    v = prev[p * 4 + tid];
  } else {
    const float s = (tid & 1) ? img / (float)H : img / (float)W;
    const int b = pr_waves_value<1, 4>(wred, 1 + tid);  // thread 0 .. 3: min x, min y, max x, max y
    v = tid < 2 ? (float)b * s - margin : (float)(b + 1) * s + margin;
    v = v < 0.0f ? 0.0f : v > img ? img : v;
  }
  boxes[p * 4 + tid] = v;
}

}  // namespace

hipError_t launch_mask_embed(const float* emb, int channels_last, const float* mask, int mask_per_image, const float* small,
                             const float* w3, const float* b3, void* keys, int P, int nb, int g, float eps, hipStream_t s) {
  if (P <= 0 || nb <= 0 || P % nb || g <= 0 || g > 64) return hipErrorInvalidValue;
  const MeGeom q = me_geom(P, nb, g, channels_last, mask_per_image);
  if (q.tiles > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mask_embed_kernel, dim3((unsigned)q.tiles), dim3(256), 0, s, emb, mask, small, w3, b3, (bf16_t*)keys, q, eps);
  return hipGetLastError();
}

hipError_t launch_prompt_tokens(const float* boxes, const float* points, const int32_t* labels, int np, const float* fixed,
                                const float* gauss, const float* corner, const float* pt_emb, const float* nap, void* tok, int P,
                                int T, float img, hipStream_t s) {
  if (P <= 0 || np < 0 || T != 5 + np + (boxes ? 2 : 1) || (int64_t)P * T * 256 > 0x7fffffff) return hipErrorInvalidValue;
  if ((np > 0 && (!points || !labels)) || ((np > 0 || !boxes) && (!pt_emb || !nap))) return hipErrorInvalidValue;
  PromptTokArgs a{boxes, points, labels, fixed, gauss, corner, pt_emb, nap, (bf16_t*)tok, P, np, T, img};
  hipLaunchKernelGGL(prompt_tokens_kernel, dim3((unsigned)((P * T * 256 + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_mask_box(const float* logits, int64_t plane_stride, const float* prev, float* boxes, int32_t* area, int P, int H,
                           int W, float img, float margin, float threshold, hipStream_t s) {
  if (P <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > 0x7fffffff || plane_stride < (int64_t)H * W) return hipErrorInvalidValue;
  const bool vec = !(W & 3) && !(plane_stride & 3) && !((uintptr_t)logits & 15);
  if (vec) hipLaunchKernelGGL(mask_box_kernel<true>, dim3((unsigned)P), dim3(256), 0, s, logits, plane_stride, prev, boxes, area, H, W, img, margin, threshold);
  else hipLaunchKernelGGL(mask_box_kernel<false>, dim3((unsigned)P), dim3(256), 0, s, logits, plane_stride, prev, boxes, area, H, W, img, margin, threshold);
  return hipGetLastError();
}

}  // namespace vdr
