// Host-side launch interface of the gfx950 kernels (internal; the public ABI is include/vdr.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <mutex>

// tuning knobs (-DVDR_TUNING builds read VDR_* environment variables): re-read on every call there, so that one
// process can alternate settings between forwards (interleaved A/B, tools/ab_forward.py); constants in the shipped build
#ifdef VDR_TUNING
#define VDR_KNOB const
constexpr bool VDR_TUNING_BUILD = true;
#else
#define VDR_KNOB static const
constexpr bool VDR_TUNING_BUILD = false;
#endif

namespace vdr {

// One-time launch state of a kernel instantiation is PER DEVICE: hipFuncSetAttribute (the > 64 KB dynamic-LDS opt-in),
// occupancy and CU counts belong to the device that is current when they are set / read.  A handle runs on its own
// device whatever device the caller has current (include/vdr.h), so a second handle on another GPU of the same process
// must find its own flags, not the first device's.
constexpr int VDR_MAX_DEVICES = 64;
static inline int current_device_index() {
  int d = -1;
  return hipGetDevice(&d) == hipSuccess && d >= 0 && d < VDR_MAX_DEVICES ? d : -1;
}
static inline int device_cu_count(int dev) {  // 0 on failure
  static int n[VDR_MAX_DEVICES] = {};
  if (dev < 0 || dev >= VDR_MAX_DEVICES) return 0;
  if (!n[dev]) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) n[dev] = prop.multiProcessorCount;
  }
  return n[dev];
}
// That state, one object per kernel instantiation (a static of its launcher).  Two host threads may launch the same kernel
// at once: steady state is one atomic load; first use takes a lock (the attribute) or asks for the same occupancy twice.
struct KernelState {
  std::atomic<int> lds_limit[VDR_MAX_DEVICES] = {};  // what hipFuncAttributeMaxDynamicSharedMemorySize was raised to (0: never)
  std::atomic<int> slots[VDR_MAX_DEVICES] = {};      // persistent kernels: workgroups of it the chip holds at once (0: not asked yet)
};
// Before a launch with `lds` bytes of dynamic LDS: above 64 KB the kernel has to opt in, once per device -- and again when
// a larger size arrives for the same kernel.  No call at or below 64 KB, none at steady state.
static inline hipError_t raise_lds_limit(KernelState& st, const void* fn, int dev, size_t lds) {
  if (lds <= 65536 || (int)lds <= st.lds_limit[dev].load(std::memory_order_acquire)) return hipSuccess;
  static std::mutex first_use;
  std::lock_guard<std::mutex> lock(first_use);
  if ((int)lds <= st.lds_limit[dev].load(std::memory_order_relaxed)) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) st.lds_limit[dev].store((int)lds, std::memory_order_release);
  return e;
}
// workgroups of `block` threads and `lds` bytes of a persistent kernel that the device holds at once; 0 on failure
static inline int persistent_slots(KernelState& st, const void* fn, int dev, int block, size_t lds) {
  int slots = st.slots[dev].load(std::memory_order_relaxed), per_cu = 0;
  const int n_cu = slots ? 0 : device_cu_count(dev);
  if (slots || n_cu <= 0 || raise_lds_limit(st, fn, dev, lds) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, block, lds) != hipSuccess || per_cu <= 0)
    return slots;
  st.slots[dev].store(per_cu * n_cu, std::memory_order_relaxed);
  return per_cu * n_cu;
}

// ---- the tile variants of launch_gemm and launch_gemm_mx: one row each, read by the launch code (gemm_launch.hip), by the
// kernel selection (gemm_kernels.h, gemm_mx.hip) and by the forward's variant choice (vdr_api.hip)
// families: ring3, ring3k (its K loop split across two wave groups of the workgroup) and ring4 (both operands staged in whole
// 128-B lines) of gemm_kernels.h, the 8-phase kernel (gemm_8p.hip), MX-fp8 operands (gemm_mx.hip: launch_gemm_mx's numbers)
enum TileFamily { TILE_RING3, TILE_RING3K, TILE_RING4, TILE_8P, TILE_MX };
// what a GemmArgs may ask of a variant (the launch refuses the rest)
enum TileCap : unsigned {
  CAP_LN_CPART = 1,     // finalises the LayerNorm partials of its rows itself (GemmArgs::ln_cpart)
  CAP_FIN_STATS = 2,    // producer-side finalisation behind the residual epilogue (GemmArgs::fin_stats)
  CAP_PATCH = 4,        // im2col-free patchify in the operand loader (GemmArgs::patch_p)
  CAP_A_RPG = 8,        // A rows gathered with two strides (GemmArgs::a_rpg)
  CAP_RESID32 = 16,     // the fp32 residual stream (GemmArgs::resid32 / C32)
  CAP_PERSISTENT = 32,  // has a persistent form (gemm_ring4p_kernel)
  RING3_CAPS = CAP_LN_CPART | CAP_A_RPG | CAP_RESID32,
  RING4_CAPS = CAP_LN_CPART | CAP_FIN_STATS | CAP_PATCH | CAP_RESID32 | CAP_PERSISTENT,
};

struct TileVariant {
  int id;
  TileFamily family;
  int waves_m, waves_n;  // a wave owns 64 x 64 of the tile (8-phase: 128 x 64)
  int depth;             // ring depth: LDS slots (ring3, MX), super-slots (ring3k), W slots (ring4), K-tile buffers (8-phase)
  unsigned caps;
  constexpr bool can(unsigned c) const { return (caps & c) == c; }
  constexpr int bm() const { return waves_m * (family == TILE_8P ? 128 : 64); }
  constexpr int bn() const { return waves_n * 64; }
  constexpr int block() const { return waves_m * waves_n * 64 * (family == TILE_RING3K ? 2 : 1); }  // threads (ring3k: two K-groups of waves)
};

// (variants 0-21, the earlier rungs of the ladder in DESIGN.md, are no longer built; 30, the persistent stream kernel of round 3, lives in tools/micro/)
constexpr TileVariant TILE_VARIANTS[] = {
    {22, TILE_RING3, 2, 4, 3, RING3_CAPS},  // 128x256, 8 waves, 3 x 24 KB, 2 WG/CU
    {23, TILE_RING3, 4, 4, 3, RING3_CAPS},  // 256x256, 16 waves, 3 x 32 KB
    {24, TILE_RING3, 2, 2, 3, RING3_CAPS},  // 128x128, 4 waves, 3 x 16 KB, 3 WG/CU
    {25, TILE_RING3K, 2, 2, 3, CAP_A_RPG},  // 128x128 tile, 8 waves = 2 K-groups x (2x2), 3 x 32 KB
    {26, TILE_RING4, 2, 4, 3, RING4_CAPS},  // 128x256, 8 waves, 2 x 16 KB (A) + 3 x 16 KB (W), 2 WG/CU
    {27, TILE_RING4, 4, 4, 3, RING4_CAPS},  // 256x256, 16 waves, 2 x 32 KB + 3 x 16 KB
    {28, TILE_RING4, 2, 2, 3, RING4_CAPS},  // 128x128, 4 waves, 2 x 16 KB + 3 x 8 KB, 2 WG/CU
    {29, TILE_RING4, 1, 2, 3, RING4_CAPS},  // 64x128, 2 waves, 2 x 8 KB + 3 x 8 KB: launches of a few hundred rows x 768 columns
    {31, TILE_8P, 2, 4, 2, 0},              // 256x256 tile, 8 waves, one persistent workgroup per CU, plain W layout
    // launch_gemm_mx's own numbering
    {0, TILE_MX, 2, 4, 3, 0},  // 128x256, 8 waves, 3 x 26 KB, 2 workgroups per CU
    {1, TILE_MX, 4, 4, 3, 0},  // 256x256, 16 waves, 3 x 36 KB
    {2, TILE_MX, 2, 2, 3, 0},  // 128x128, 4 waves, 3 x 17 KB, 3 workgroups per CU
};
constexpr const TileVariant* tile_variant(int id, bool mx = false) {  // null: no such variant
  for (const TileVariant& r : TILE_VARIANTS)
    if (r.id == id && (r.family == TILE_MX) == mx) return &r;
  return nullptr;
}
constexpr int VARIANT_RING3_128x256 = 22, VARIANT_RING3_128x128 = 24, VARIANT_8P = 31;  // the variants other code names

// row r of a compact [R, *] view  <->  row (r / rpg) * gstride + off + (r % rpg) of a token buffer
struct RowMap {
  int rpg;
  int64_t gstride;
  int off;
};
static inline RowMap identity_map() { return RowMap{1 << 30, 0, 0}; }

enum Epilogue { EPI_BIAS = 0, EPI_BIAS_GELU = 1, EPI_BIAS_RESID = 2, EPI_SWIGLU = 3, EPI_PATCH = 4,
                // internal to gemm_mx.hip: GELU / SwiGLU with the output re-quantised to MX-fp8
                EPI_BIAS_GELU_MX = 5, EPI_SWIGLU_MX = 6,
                // internal to build_gemm_launch: EPI_BIAS_RESID with the residual stream kept in fp32 (GemmArgs::resid32 / C32)
                EPI_BIAS_RESID32 = 7,
                // EPI_BIAS_GELU with another activation (vdr_dev.h): QuickGELU (CLIP) and tanh-GELU (SigLIP).  The public
                // vdr_epilogue values are these numbers
                EPI_BIAS_QGELU = 8, EPI_BIAS_TGELU = 9 };
// the epilogues "bias, then an elementwise activation, bf16 out": they share every kernel path of EPI_BIAS_GELU
constexpr bool epi_is_act(int e) { return e == EPI_BIAS_GELU || e == EPI_BIAS_QGELU || e == EPI_BIAS_TGELU; }

struct GemmArgs {
  const void* A;      // [M, K] bf16, row stride lda
  const void* W;      // [N, K] bf16 (PyTorch Linear layout), row stride ldw; or the packed form (w_interleaved)
  int w_interleaved = 0;  // W is [N/2][K/32][2][32] (launch_w_interleave): whole-line operand loads, gemm_kernels.h
  const float* bias;  // [N] or null
  const void* resid;  // [*, ldr] bf16 (EPI_BIAS_RESID), indexed by the OUTPUT row
  // vdr_config.resid_fp32 (ring3 / ring4 kernels, EPI_BIAS_RESID): the residual is READ from resid32 [*, ldr] fp32 instead of
  // `resid`, the fp32 sum is written to C32 [*, ldc] fp32 AND, rounded once, to C (the bf16 copy the next GEMM multiplies)
  const float* resid32 = nullptr;
  float* C32 = nullptr;
  // rows of A (and of ln_stats) that are READABLE memory, >= M (0 = M).  Tile variant 31 loads whole 256-row tiles: it takes
  // a ragged M only when the buffers are readable up to M rounded up to 256 (the forward's workspace is); rows past M are
  // never stored (the store descriptor ends after row M - 1)
  int64_t a_rows = 0;
  const float* gamma; // [N] LayerScale or null
  const float* pos;   // [tokens, N] fp32 (EPI_PATCH), indexed by off + r % rpg
  void* C;            // bf16, row stride ldc
  int64_t M;
  int N, K;
  int64_t lda, ldw, ldc, ldr;
  RowMap omap;        // output row map (EPI_PATCH); identity otherwise
  // LayerNorm folded into the GEMM (pre-LN models):
  //   consumer side: y = r_m * (x.W'^T - mu_m * colsum) + bias', with (mu_m, r_m) = ln_stats[m]
  const float* ln_stats = nullptr;  // [M][2] fp32 (mean, rstd) or null
  const float* colsum = nullptr;    // [N] fp32: sum_k W'[n][k]
  //   consumer side, statistics finalised inside the GEMM (ring3 variants 22-24, up to 16 groups): the producers'
  //   partials instead of ln_stats; (mean, rstd) = what ln_finalize_kernel computes from them, bit for bit
  const float* ln_cpart = nullptr;  // [ln_groups][ln_cstride][2] fp32 or null
  int ln_groups = 0;
  int64_t ln_cstride = 0;
  float ln_eps = 0.0f;  // (D = 64 * ln_groups)
  // producer side, ring4 tile variants with the residual epilogue: the workgroup that stores the LAST partial sums of a
  // block of tile rows turns them into (mean, rstd) at fin_stats [M][2] -- ln_finalize_kernel's arithmetic, no launch.
  // fin_cnt: one zeroed counter per tile row (left zeroed); the partials span fin_groups = N / 64 groups
  float* fin_stats = nullptr;
  uint32_t* fin_cnt = nullptr;
  float fin_eps = 0.0f;
  //   producer side: per output row and 64-column group, (sum, sum of squares) of the bf16 outputs
  float* ln_part = nullptr;         // [N/64][part_stride][2] fp32 or null
  int64_t part_stride = 0;
  // SAM window un-partition on the OUTPUT rows: GEMM row m is a token of a ws x ws window (windows
  // row-major over the zero-padded grid); it lands at token (y, x) of the g x g grid, padding is dropped
  int win_ws = 0, win_g = 0;
  // A rows gathered with two strides: row m starts at element (m / a_rpg) * a_gs + (m % a_rpg) * a_is
  // (a_rpg = 0: plain m * lda).  Used to read the per-head q slices of a packed qkv activation as rows.
  int a_rpg = 0;
  int64_t a_gs = 0, a_is = 0;
  int out_f32 = 0;  // C is fp32 (EPI_BIAS / EPI_PATCH)
  // im2col-free patchify (EPI_PATCH on the ring4 variants): A = bf16 NCHW images [B, C, g*p, g*p], M = B*g*g tokens,
  // K = C*p*p with p in {8, 16, 32}; the operand loader gathers 16-byte runs of pixels straight from the images
  int patch_p = 0, patch_g = 0, patch_C = 0;
  // MX-fp8 GEMM (launch_gemm_mx): A and W are e4m3 payloads, *_scale their e8m0 scale arrays (mx.hip layout)
  const void* a_scale = nullptr;
  const void* w_scale = nullptr;
  void* c_scale = nullptr;  // non-null: C is written as MX-fp8 (payload [M][ldc] bytes + scales), not bf16
};

hipError_t launch_gemm(const GemmArgs& a, int epilogue, int variant, hipStream_t s);
// whether tile variant 31 (gemm_8p.hip: the 256 x 256 x 64 8-phase kernel, one workgroup per CU) takes this launch: EPI_BIAS /
// an activation epilogue (EPI_BIAS_GELU / _QGELU / _TGELU) with a plain bf16 output, plain weight layout, N % 256 == 0, K % 128 == 0, M % 256 == 0 or a_rows covering the
// last 256-row tile, at least 2 tiles per CU with the last round of workgroups at least 85 % full
bool gemm_8p_eligible(const GemmArgs& a, int epilogue);
bool gemm_8p_shape_ok(int64_t M, int N);  // its tile-count rule alone
// rounds of one workgroup per CU such a launch runs (0: the rule refuses the shape); idle: the fraction of a round its last one leaves empty
int64_t gemm_8p_rounds(int64_t M, int N, double* idle = nullptr);
// [N][K] bf16 (row stride ld elements) -> the pair-interleaved weight layout (N even, K % 32 == 0)
hipError_t launch_w_interleave(const void* src, void* dst, int N, int K, int64_t ld, hipStream_t s);

// y[r] = LN(x[imap(r)]) ; optional cls source: rows with r % cls_period == 0 read cls (fp32 [D])
struct LnArgs {
  const void* x;
  int in_bf16;
  void* y;
  int out_bf16;
  const float* gamma;
  const float* beta;
  int64_t rows;  // output rows
  int D;
  float eps;
  RowMap imap;
  RowMap omap;
  const float* cls;  // or null
  int cls_period;
  // SAM window partition on the OUTPUT rows (input rows are tokens of a g x g grid, row-major)
  int win_ws = 0, win_g = 0;
  int64_t ldy = 0;  // elements between consecutive output rows (0 = D): column slices of a wider matrix
};
hipError_t launch_layernorm(const LnArgs& a, hipStream_t s);

//   out_scale != NULL: `out` is written as MX-fp8 (payload [batch*seq][heads*64] bytes + e8m0 scales), the
//   operand of the fp8 out-projection
hipError_t launch_attention(const void* qkv, void* out, int batch, int seq, int heads, int variant,
                            hipStream_t s, void* out_scale = nullptr, const int* lens = nullptr, int len_add = 0,
                            int head_dim = 64);
//   lens != NULL: entry b attends over its first lens[b] + len_add rows only (sequences padded to seq)
//   head_dim: 64 (attention.hip), or 32 / 96 / 128 (attention_hd.hip: bf16 out only, every variant the same kernel);
//   qkv [batch*seq, 3*heads*head_dim], out [batch*seq, heads*head_dim]
hipError_t launch_attention_hd(const void* qkv, void* out, int batch, int seq, int heads, int head_dim, hipStream_t s,
                               const int* lens, int len_add);
// attention maps (attention_probs.hip): softmax(q k^T dh^-1/2) of the first q_rows query rows of every (sequence, head)
// of the same qkv; out [batch, heads, q_rows, seq] (head_mean = 0) or [batch, q_rows, seq] (1, mean over the heads),
// fp32 or bf16 (out_bf16).  head_dim 32 / 64 / 96 / 128, 1 <= q_rows <= seq
hipError_t launch_attention_probs(const void* qkv, void* out, int batch, int seq, int heads, int head_dim, int q_rows,
                                  int head_mean, int out_bf16, hipStream_t s);

// one-query attention pooling (attention_pool.hip): out[b, h*dh + d] = sum_j softmax_j(q_h . k[b, j, h] dh^-1/2) v[b, j, h, d];
// q fp32 [heads * head_dim] (one probe for the whole batch), kv bf16 rows b * n + j of ldkv elements, [k | v] columns,
// out bf16 [batch, heads * head_dim].  head_dim 32 / 64 / 96 / 128, n >= 1, ldkv % 8 == 0, kv 16-byte aligned
// csrc/mask_decoder.hip: the kernels of SAM's mask decoder (include/vdr.h)
hipError_t launch_cross_attention(const void* q, int64_t ldq, const float* q_add, const void* k, int64_t ldk, const float* k_add,
                                  const void* v, int64_t ldv, void* out, int64_t ldo, int problems, int tq, int tk, int heads,
                                  int head_dim, hipStream_t s);
hipError_t launch_token_linear(const void* x, int64_t ldx, const void* x_add, int64_t ldxa, const void* W, const float* bias,
                               const void* resid, int64_t ldr, void* y, int out_f32, int64_t ldy, int M, int N, int K, int groups,
                               int relu, hipStream_t s, int x_rpg = 0, int64_t x_gs = 0);
hipError_t launch_decoder_setup(const float* boxes, const float* fixed, const float* gauss, const float* corner, const float* emb,
                                int channels_last, const float* no_mask, void* tok, void* keys, int B, int nb, int g, float img, hipStream_t s);
hipError_t launch_mask_upscale(const void* x, const void* W, const float* bias, const float* hyper, float* out, int problems,
                               int g, int gelu_in, hipStream_t s);
hipError_t launch_decoder_keys(const float* emb, int channels_last, const float* no_mask, void* keys, int B, int nb, int g, hipStream_t s);
// csrc/mask_prompt.hip: point / mask prompts and the box of a mask (include/vdr.h "mask prompt ops")
constexpr int MASK_EMBED_SMALL = 332;  // the packed fp32 weights of mask_downscaling.{0,1,3,4}: w1 [4,4] b1 g1 e1 [4] w2 [16,16] b2 g2 e2 [16]
hipError_t launch_mask_embed(const float* emb, int channels_last, const float* mask, int mask_per_image, const float* small,
                             const float* w3, const float* b3, void* keys, int P, int nb, int g, float eps, hipStream_t s);
hipError_t launch_prompt_tokens(const float* boxes, const float* points, const int32_t* labels, int np, const float* fixed,
                                const float* gauss, const float* corner, const float* pt_emb, const float* nap, void* tok, int P,
                                int T, float img, hipStream_t s);
hipError_t launch_mask_box(const float* logits, int64_t plane_stride, const float* prev, float* boxes, int32_t* area, int P, int H,
                           int W, float img, float margin, float threshold, hipStream_t s);
// csrc/mask_stats.hip, csrc/nms.hip: the post-processing of the automatic mask generator (include/vdr.h "automatic mask generation")
size_t mask_stats_workspace_bytes(int P, int H, int W, int oh, int ow);  // 0: a shape the op refuses
hipError_t launch_mask_stats(const float* logits, int64_t plane_stride, int group, int64_t group_stride, int P, int H, int W, int oh, int ow,
                             float threshold, float offset, void* work, int32_t* counts, int32_t* box, hipStream_t s);
constexpr int NMS_MAX_BOXES = 4096;  // 64 words of 64 bits: one lane of the walking wave per word
size_t nms_workspace_bytes(int n);
hipError_t launch_nms(const float* boxes, const int32_t* order, int n, float iou_threshold, void* work, uint8_t* keep, int32_t* kept,
                      int32_t* count, hipStream_t s);
// csrc/components.hip: connected components of mask planes (include/vdr.h "connected components"; the mapping is components_map.h)
size_t components_workspace_bytes(int P, int H, int W, int clean);  // 0: a shape the ops refuse; clean: vdr_op_mask_clean's
hipError_t launch_connected_components(const uint8_t* mask, int P, int H, int W, int connectivity, int value, void* work, int32_t* root,
                                       int32_t* area, int32_t* count, hipStream_t s);
hipError_t launch_mask_clean(const uint8_t* mask, int P, int H, int W, int min_area, int connectivity, int mode, void* work, uint8_t* out,
                             int32_t* changed, int32_t* stats, hipStream_t s);
hipError_t launch_mask_binarize(const float* logits, int64_t plane_stride, int group, int64_t group_stride, int P, int H, int W, int oh, int ow,
                                float threshold, uint8_t* out, hipStream_t s);
// csrc/edt.hip: exact Euclidean distance transform of mask planes (include/vdr.h "distance transform"; the mapping is edt_map.h)
size_t distance_transform_workspace_bytes(int P, int H, int W);  // 0: a shape the op refuses
hipError_t launch_distance_transform(const uint8_t* mask, int P, int H, int W, int value, int outside, int r2, void* work, int32_t* d2,
                                     int32_t* nearest, int32_t* peak, uint8_t* within, hipStream_t s);
// csrc/edt3d.hip: exact 3-D Euclidean distance transform with integer voxel spacing (include/vdr.h; the mapping is edt3d_map.h)
size_t distance_transform_3d_workspace_bytes(int P, int Z, int H, int W);  // 0: a shape the op refuses
hipError_t launch_distance_transform_3d(const uint8_t* vol, int P, int Z, int H, int W, int qz, int qy, int qx, int value, int outside,
                                        int64_t r2, void* work, int64_t* d2, int64_t* peak, uint8_t* within, hipStream_t s);
hipError_t launch_attention_pool(const float* q, const void* kv, int64_t ldkv, void* out, int batch, int n, int heads,
                                 int head_dim, hipStream_t s);

// SAM / MedSAM decomposed relative position bias (attention_relpos.hip)
//   qkv rows are S*S-token windows (or whole grids) back to back
//   table [Npad][64] bf16: rows [0, 2S-1) = rel_pos_h, rows [Npad/2, Npad/2 + 2S-1) = rel_pos_w, rest zero;
//   Npad = relpos_npad(S).  T = q . table^T is one GEMM over (token, head) rows (launch_gemm with a_rpg).
// ---- MX-fp8 (mx.hip, gemm_mx.hip) ---------------------------------------------------------------------
static inline int64_t mx_rows_pad(int64_t rows) { return (rows + 255) / 256 * 256; }
static inline size_t mx_scale_bytes(int64_t rows, int K) { return (size_t)mx_rows_pad(rows) * (size_t)(K / 32); }
//   bf16 [rows][K] (row stride ldx elements) -> e4m3 payload [rows][K] + e8m0 scales
hipError_t launch_mx_quant(const void* x, int64_t rows, int K, int64_t ldx, void* q, void* scales, hipStream_t s);
hipError_t launch_mx_dequant(const void* q, const void* scales, int64_t rows, int K, float* y, hipStream_t s);
//   LayerNorm over bf16 rows, MX out
//   win_ws > 0: output rows in SAM window-partition order (out_rows = rows of that padded layout)
hipError_t launch_ln_mx(const void* x, const float* gamma, const float* beta, float eps, int64_t rows, int D, void* q,
                        void* scales, hipStream_t s, int win_ws = 0, int win_g = 0, int64_t out_rows = 0);
//   C = epi(A . W^T) with MX operands; variant 0: 128x256 tile / 8 waves, 1: 256x256 / 16 waves, 2: 128x128 / 4 waves
hipError_t launch_gemm_mx(const GemmArgs& a, int epilogue, int variant, hipStream_t s);

// ---- pre/post-processing (prep.hip) --------------------------------------------------------------------
size_t prepare_scratch_bytes(int batch, int h, int w, int ch, int out_side);
hipError_t launch_prepare(const void* src, int src_f32, int batch, int h, int w, int ch, int64_t sb, int64_t sy, int64_t sx,
                          int64_t sc, int flip, int out_side, void* out, int out_bf16, float* scratch, hipStream_t s);
hipError_t launch_window_ct(const void* ct, int in_i16, int64_t n, double width, double level, float* out, hipStream_t s);
hipError_t launch_hu_to_rgb(const void* hu, int dtype, int64_t n, void* rgb, hipStream_t s);
hipError_t launch_crop_hwc(const float* src, float* dst, int batch, int H, int W, int C, int y0, int x0, int ch, int cw,
                           hipStream_t s);
// scipy.ndimage.affine_transform(order=3, mode='nearest', prefilter=True) on every (H, W) plane of an [H, W, planes]
// volume (rotate.hip); dtype 0 f64, 1 f32, 2 u8 (boolean mask, truncating store); scratch = affine_cubic_scratch_bytes
hipError_t launch_voxel_sequence(const float* feat, const int64_t* index, const double* xyz, const double* expo, int64_t n,
                                 int D, void* out, int out_dtype, hipStream_t s);
size_t affine_cubic_scratch_bytes(int H, int W, int64_t planes);
hipError_t launch_affine_cubic(const void* src, int dtype, int H, int W, int64_t planes, const double* matrix,
                               const double* offset, void* out, int clip01, double* scratch, hipStream_t s);

static inline int relpos_npad(int S) { return 2 * ((2 * S - 1 + 31) / 32 * 32); }
hipError_t launch_relpos_pack(const float* rel_h, const float* rel_w, void* table, int S, hipStream_t s);
//   softmax(q k^T / 8 + T[qh - kh + S-1] + T[Npad/2 + qw - kw + S-1]) v per (window, head);
//   T fp32 [batch*S*S*heads][Npad]; S in {4, 7, 10, 14} single pass, 64 chunked, every other S <= 64 the run-time-grid
//   kernel (attn_relpos_any_kernel).  any_variant (tuning / measurements): 1 / 2 force that kernel, single / double
//   buffered, at any S
hipError_t launch_attention_relpos(const void* qkv, const float* T, void* out, int batch, int S, int heads,
                                   hipStream_t s, int any_variant = 0);
//   rel-pos table resampling (pos_interp.hip): get_rel_pos of segment_anything, i.e. F.interpolate(mode="linear",
//   align_corners=False) along the rows of table [L0][D] -> out [L][D]; fp64 arithmetic, one rounding to fp32
hipError_t launch_relpos_interp(const float* table, int L0, int D, float* out, int L, hipStream_t s);

// 3x3 / pad 1 im2col over NHWC tokens of a g x g grid: col[r][j*C + c] = y[(y+ky-1, x+kx-1)][c], j = ky*3 + kx
hipError_t launch_im2col3(const void* y, void* col, int batch, int g, int C, hipStream_t s);

// images NCHW [batch, C, H, W] -> col [batch*n, Kp] bf16, n = (H / p) * (W / p) patches in (py, px) order, with
// k = c*p*p + ky*p + kx, zero padded to Kp
hipError_t launch_im2col(const void* images, int in_bf16, void* col, int batch, int C, int H, int W, int p,
                         int Kp, hipStream_t s);
// the same for Conv2d(kernel=p, stride=s), s | p (patch_stride.hip): n = ((H - p) / s + 1) * ((W - p) / s + 1) overlapping
// patches, patch (py, px) starting at pixel (py*s, px*s); s == p is launch_im2col
hipError_t launch_im2col_strided(const void* images, int in_bf16, void* col, int batch, int C, int H, int W, int p, int s,
                                 int Kp, hipStream_t st);

// Log-binned descriptors (log_bin.hip): out [batch, gh*gw, (1 + 8*hierarchy)*C] from F read in place (patch rows ld
// elements apart, images image_stride apart, bf16 or fp32); work: fp32 [(hierarchy-1)*batch*gh*gw*C] for the level means
// (three or fewer box-sum launches in front of the copy).  C % 8 == 0; x, work, out and every row 16-byte aligned.
hipError_t launch_log_bin(const void* x, int in_bf16, int64_t ld, int64_t image_stride, int batch, int gh, int gw, int C,
                          int hierarchy, float* work, void* out, int out_bf16, hipStream_t st);

// The row norms of the two-sided cosine ops (the kernel is in nn_cosine.hip; local_corr.hip launches it too):
// rn(v) = 1 / max(sqrt(sum v^2), 1e-8), IEEE sqrt and division, of every row of side X, then of side Y, in one launch of one
// wave per row.  A side is `pairs` maps of t bf16 rows of d channels, rows ld elements apart, problems ps apart (0 allowed);
// rn is [pairs][t_pad].  t == 0 (a CosSide{}): no such side.
struct CosSide {
  const void* x = nullptr;
  int64_t ld = 0, ps = 0;
  int t = 0, t_pad = 0;
  float* rn = nullptr;
};
hipError_t launch_cosine_rnorm(const CosSide& X, const CosSide& Y, int d, int pairs, hipStream_t st);

// Cosine nearest neighbours of two descriptor maps (nn_cosine.hip; the definition is vdr_op_nn_cosine's in include/vdr.h):
// X_p [tx, d], Y_p [ty, d] bf16, rows ldx / ldy elements apart, pairs x_stride / y_stride apart (0: one map against many).
// d % 32 == 0; pointers, row and pair strides 16-byte aligned; work: nn_cosine_work_bytes(pairs, tx, ty) bytes.  col_sim and
// col_idx both null: the column side is skipped.  Three launches (row norms, the fused tile kernel, the fold of partials).
size_t nn_cosine_work_bytes(int pairs, int tx, int ty);
hipError_t launch_nn_cosine(const void* x, int64_t ldx, int64_t x_stride, int tx, const void* y, int64_t ldy, int64_t y_stride,
                            int ty, int pairs, int d, void* work, float* row_sim, int32_t* row_idx, float* col_sim,
                            int32_t* col_idx, hipStream_t st);

// k nearest neighbours of two descriptor maps (knn.hip; the definition is vdr_op_knn's in include/vdr.h): operands as
// launch_nn_cosine's, X the queries and Y the candidates; k 1 .. 16, l2 != 0: squared distances instead of cosines;
// exclude_diag: candidate i is not eligible for query i; tc - exclude_diag >= k.  val / idx [pairs][tq][k], best first; work:
// knn_work_bytes(pairs, tq, tc, k) bytes.  Three launches (row norms or sums of squares, the fused tile kernel, the merge of
// the partial lists); every index is knn_map.h's.
size_t knn_work_bytes(int pairs, int tq, int tc, int k);
hipError_t launch_knn(const void* x, int64_t ldx, int64_t x_stride, int tq, const void* y, int64_t ldy, int64_t y_stride, int tc,
                      int pairs, int d, int k, int l2, int exclude_diag, void* work, float* val, int32_t* idx, hipStream_t st);

// Windowed correlation of two descriptor maps on one gh x gw grid (local_corr.hip; the definition is
// vdr_op_local_correlation's in include/vdr.h): operands as launch_nn_cosine's with tx = ty = gh * gw; radius 1 .. 8.
// cost [pairs][t][(2r+1)^2] fp32 and / or (best_sim, best_idx) [pairs][t]; work: local_correlation_work_bytes(...) bytes.
// Two launches (row norms, the tile kernel), a third (the fold over the window) when the best pair is asked for.
size_t local_correlation_work_bytes(int pairs, int gh, int gw, int radius);
hipError_t launch_local_correlation(const void* x, int64_t ldx, int64_t x_stride, const void* y, int64_t ldy, int64_t y_stride,
                                    int pairs, int gh, int gw, int d, int radius, int transposed, void* work, float* cost,
                                    float* best_sim, int32_t* best_idx, hipStream_t st);

// Multi-source soft window vote (window_vote.hip; the definition is vdr_op_window_vote's in include/vdr.h): cost
// [problems][sources][t][(2r+1)^2] and src [problems][sources][t][n_classes] fp32 -> scores [problems][t][n_classes], and
// optionally labels [problems][t], (idx, val) [problems][t][k].  One launch, a wave per query, no scratch memory.
hipError_t launch_window_vote(const float* cost, const float* src, int problems, int sources, int gh, int gw, int radius, int k,
                              int n_classes, int weights, float temperature, float* scores, int32_t* labels, int32_t* idx,
                              float* val, hipStream_t st);

// Thresholded affinity graphs of descriptor maps, one bit per pair (affinity.hip; the definitions are vdr_op_affinity_bits' and
// vdr_op_bits_matvec's in include/vdr.h): X_p [t, d] bf16, rows ldx elements apart, problems x_stride apart (0 allowed);
// d % 32 == 0; pointers and strides 16-byte aligned; work: affinity_work_bytes(pairs, t) bytes; bits [pairs][t][pitch] with
// pitch == affinity_pitch(t).  Two launches (row norms, the fused tile kernel); the matvec is one.
int affinity_pitch(int t);
size_t affinity_work_bytes(int pairs, int t);
hipError_t launch_affinity_bits(const void* x, int64_t ldx, int64_t x_stride, int t, int pairs, int d, float tau, int exclude_diag,
                                void* work, uint32_t* bits, int pitch, hipStream_t st);
hipError_t launch_bits_matvec(const uint32_t* bits, int pitch, int t, int pairs, const float* v, int nv, float* y, int32_t* degree,
                              hipStream_t st);

// PCA of dense descriptor maps (pca.hip; the definitions are vdr_op_col_mean's, vdr_op_covariance's and vdr_op_pca_project's
// in include/vdr.h): `problems` problems of `imgs` images of t rows of d channels, bf16 or fp32, rows ld and images
// image_stride elements apart.  d % 32 == 0, d <= 2048; pointers and strides 16-byte aligned; work: pca_work_bytes(...)
// bytes.  Two launches each (partials, fold); the projection a third when it rescales.
size_t pca_work_bytes(int problems, int imgs, int t, int d);
hipError_t launch_col_mean(const void* x, int in_bf16, int64_t ld, int64_t image_stride, int problems, int imgs, int t, int d,
                           void* work, float* mean, hipStream_t st);
hipError_t launch_covariance(const void* x, int in_bf16, int64_t ld, int64_t image_stride, int problems, int imgs, int t, int d,
                             const float* mean, void* work, float* cov, hipStream_t st);
hipError_t launch_pca_project(const void* x, int in_bf16, int64_t ld, int64_t image_stride, int problems, int imgs, int t, int d,
                              const float* mean, const float* comps, int k, int scale, void* work, float* proj, float* minmax,
                              hipStream_t st);

// The Gram side and the top-k solver (pca.hip, pca_topk.hip; the definitions are vdr_op_gram's, vdr_op_pca_back_project's and
// vdr_op_sym_topk's in include/vdr.h).  Per image only (imgs = 1); d % 32 == 0 with no upper bound, 2 <= t <= 4096.
// launch_col_mean_any: launch_col_mean's kernels and bits at any d.
size_t pca_topk_side_work_bytes(int problems, int t, int d, int k);
hipError_t launch_col_mean_any(const void* x, int in_bf16, int64_t ld, int64_t image_stride, int problems, int t, int d, void* work,
                               float* mean, hipStream_t st);
hipError_t launch_gram(const void* x, int in_bf16, int64_t ld, int64_t image_stride, int problems, int t, int d, const float* mean,
                       void* work, float* gram, hipStream_t st);
hipError_t launch_pca_back_project(const void* x, int in_bf16, int64_t ld, int64_t image_stride, int problems, int t, int d,
                                   const float* mean, const float* u, const float* values, int k, void* work, float* comps,
                                   hipStream_t st);
size_t sym_topk_work_bytes(int problems, int n);
hipError_t launch_sym_topk(const float* a, int problems, int n, int k, float tol, int max_iter, void* work, float* values,
                           float* vectors, int32_t* iters, float* resid, hipStream_t st);

// Lloyd's k-means over bf16 descriptor maps (kmeans.hip; the definitions are vdr_op_kmeans_assign's and vdr_op_kmeans_update's
// in include/vdr.h): `problems` problems of `imgs` images of t rows of d channels, rows ld, images image_stride and problems
// problem_stride elements apart.  d % 32 == 0, 1 <= k <= min(1024, R); pointers and strides 16-byte aligned; active: null or
// [problems] flags (0: the problem is skipped); work: kmeans_work_bytes(...) bytes.  Assign: three launches (norms, the fused
// tile kernel, inertia / changed); update: two (partial sums, fold and division).
size_t kmeans_work_bytes(int problems, int imgs, int t, int d, int k);
hipError_t launch_kmeans_assign(const void* x, int64_t ld, int64_t image_stride, int64_t problem_stride, int problems, int imgs,
                                int t, int d, int k, const float* centroids, const int32_t* active, void* work, int32_t* labels,
                                float* min_dist, float* inertia, int32_t* changed, hipStream_t st);
hipError_t launch_kmeans_update(const void* x, int64_t ld, int64_t image_stride, int64_t problem_stride, int problems, int imgs,
                                int t, int d, int k, const int32_t* labels, const int32_t* active, void* work, float* centroids,
                                int32_t* counts, hipStream_t st);

// Squared Mahalanobis distances of bf16 descriptor rows (mahalanobis.hip; the definition is vdr_op_mahalanobis' in
// include/vdr.h): the k-means operand; the model of problem p at mean + p * mean_stride ([d] fp32) and whiten + p * whiten_stride
// ([k][d] fp32), a stride of 0 shares it.  d % 32 == 0, 1 <= k <= VDR_MAHALANOBIS_MAX_K; x, mean, whiten and the strides 16-byte
// aligned; d2 [problems][R] fp32.  One launch, no scratch.
hipError_t launch_mahalanobis(const void* x, int64_t ld, int64_t image_stride, int64_t problem_stride, int problems, int imgs,
                              int t, int d, const float* mean, int64_t mean_stride, const float* whiten, int64_t whiten_stride,
                              int k, float* d2, hipStream_t st);

// Joint bilateral upsampling of descriptor maps (upsample.hip; the definitions are vdr_op_guide_lowres' and
// vdr_op_upsample_guided's in include/vdr.h): features [batch][gh][gw][C] read through ld / image_stride, guide
// [batch][Cg][H][W] contiguous, H = p + (gh - 1) s, box [y0, y1) x [x0, x1) inside the image, out [batch][y1 - y0][x1 - x0][C].
// C % 8 == 0, radius 1..3, Cg 1..4, s | p; features and strides 16-byte aligned; work: upsample_work_bytes(...) bytes.  Two
// launches: the low-resolution guide of the patches the box reaches, then the tile kernel.
size_t upsample_work_bytes(int batch, int Cg, int gh, int gw);
hipError_t launch_guide_lowres(const void* guide, bool guide_bf16, int batch, int Cg, int H, int W, int p, int s, int gh, int gw,
                               float* work, hipStream_t st);
hipError_t launch_upsample_guided(const void* f, bool f_bf16, int64_t ld, int64_t image_stride, int batch, int gh, int gw, int C,
                                  const void* guide, bool guide_bf16, int Cg, int H, int W, int p, int s, int radius, float cs,
                                  float cr, const float* conf, int y0, int x0, int y1, int x1, float* work, void* out, bool out_bf16,
                                  hipStream_t st);

// pos_embed resampling (pos_interp.hip): the patch rows of a position table from a gh0 x gw0 grid to gh x gw, bicubic
// (A = -0.75, align_corners = False, border taps clamped), fp64 arithmetic, one rounding to fp32
hipError_t launch_pos_interp(const float* pos, int gh0, int gw0, int D, float* out, int gh, int gw, hipStream_t s);

// DINOv3 2-D RoPE (rope.hip).  Table: cos / sin [gh*gw][head_dim/2] fp32 of the axial angles, fp64 arithmetic, one rounding
// (load time).  Rotation: q and k of rows b*seq + prefix + j (j < seq - prefix) of qkv [batch*seq][3*heads*head_dim] bf16 in
// place, table row j; prefix rows and v untouched.  head_dim in {32, 64, 128}; 16-byte aligned pointers.
hipError_t launch_rope2d_table(int gh, int gw, int head_dim, float theta, float* cos_out, float* sin_out, hipStream_t s);
hipError_t launch_rope2d(void* qkv, int batch, int seq, int prefix, int heads, int head_dim, const float* cos_t,
                         const float* sin_t, hipStream_t s);

// prefix rows of an image model (bf16 out): x[b*row_stride + 0][:] = cls + pos[0]; x[b*row_stride + 1 + r][:] = reg[r],
// r < n_reg (register tokens: no position; reg may be null when n_reg == 0)
hipError_t launch_prefix_rows(const float* cls, const float* pos, const float* reg, int n_reg, void* x, int batch,
                              int64_t row_stride, int D, hipStream_t s);

// token assembly for the token model: x[b*(S+1)+1+i] = tok[b*S+i] (+pos), x[b*(S+1)] = cls (+pos[0]); bf16 out
hipError_t launch_assemble_tokens(const void* tok, int in_bf16, const float* cls, const float* pos,
                                  void* x, int batch, int seq, int D, int has_cls, hipStream_t s);

// LayerNorm statistics kept apart from the normalisation (the normalisation itself is folded into
// the consuming GEMM): part [groups][stride][2] (sum, sumsq per 64-column group) -> stats [rows][2]
// (mean, rstd)
hipError_t launch_ln_finalize(const float* part, int groups, int64_t stride, float* stats, int64_t rows, int D,
                              float eps, hipStream_t s);
// as launch_prefix_rows, plus the (sum, sumsq) partials of each of the 1 + n_reg rows it writes
hipError_t launch_prefix_rows_stats(const float* cls, const float* pos, const float* reg, int n_reg, void* x, float* part,
                                    int64_t part_stride, int batch, int64_t row_stride, int D, hipStream_t s);

// x[r] = LN(x[r]) in place over bf16 rows [rows, D], plus the (sum, sumsq) partials of the normalised bf16 rows in the
// fold's layout part [D/64][part_stride][2] (vdr_config.input_ln with the LayerNorm fold on); D % 64 == 0
hipError_t launch_ln_rows_stats(void* x, const float* gamma, const float* beta, float eps, int64_t rows, int D, float* part,
                                int64_t part_stride, hipStream_t s);

// y[r] = x[imap(r)], bf16 -> bf16 / fp32
hipError_t launch_gather_rows(const void* x, void* y, int out_bf16, int64_t rows, int D, RowMap imap,
                              hipStream_t s, int in_f32 = 0, int64_t ldy = 0, int64_t ldx = 0);

// Mean over the patch rows of each image, of the final-normalised (norm = 1: LayerNorm with gamma / beta, the arithmetic
// of the LayerNorm kernel) or raw (norm = 0) residual stream: x rows b*ntok + ncls + j, j < n, of `batch` images ->
// y + b*ldy [D] (bf16 or fp32).  Two deterministic passes, no atomics: fp32 partial sums per fixed chunk of
// POOL_CHUNK rows into part [batch][ceil(n / POOL_CHUNK)][D], then their sum in chunk order times 1/n.
constexpr int POOL_CHUNK = 64;
inline size_t pool_part_bytes(int batch, int n, int D) { return (size_t)batch * ((n + POOL_CHUNK - 1) / POOL_CHUNK) * D * 4; }
hipError_t launch_pool_rows(const void* x, int in_bf16, int norm, const float* gamma, const float* beta, float eps, int batch,
                            int ntok, int ncls, int n, int D, float* part, void* y, int out_bf16, int64_t ldy, hipStream_t s);

}  // namespace vdr
