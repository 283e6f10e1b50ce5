/*
 * vdr.h — C ABI of libvdr.so, the MI355X-native (gfx950) ViT dense-descriptor /
 * CLS-feature forward path for the larosi/vit-deep-radiomics pipeline.
 *
 * The reference has no FFI of its own: its boundary for this path is the
 * torch.nn.Module call protocol at three sites:
 *
 *   R1  src/tfds_dense_descriptor.py:51-67    model = load_model(name, path); model.model_name
 *   R2  src/tfds_dense_descriptor.py:122-129  model.image_encoder(x) / model.patch_embed(x)
 *   R3  src/models_archs.py:141-147           model(x[B,S,D]) -> (logits[B,C], cls[B,D])
 *
 * Every entry point below says which of those call sites (or which torch op
 * invoked underneath them) it replaces.  The Python shim in
 * vit-deep-radiomics_amd/vdr/ binds these symbols with ctypes and re-creates
 * R1-R3 on top of them (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / C++ types cross this boundary;
 *   - every function returns 0 on success or a negative vdr_status; nothing
 *     throws; vdr_last_error() gives the text of the last failure on a handle
 *     (or of the last failure of a handle-less call when passed NULL);
 *   - device pointers are gfx950 HBM addresses of the device the handle was
 *     created on; the caller owns inputs, outputs and the workspace and keeps
 *     them alive until the stream has drained; the library owns only its packed
 *     weights;
 *   - all work is enqueued on the hipStream_t passed as `void* stream`
 *     (NULL = the null stream); the hot-path calls (vdr_forward*, vdr_op_*) never
 *     synchronise the device, allocate or copy from the host: they can be captured
 *     into a HIP graph from the first call on.  The load-time calls
 *     (vdr_set_weight, vdr_finalize) are synchronous;
 *   - a handle's calls run on the handle's device whatever device is current, and
 *     leave the caller's current device unchanged;
 *   - a handle is bound to one device and is not thread-safe (one per rank); several handles on DIFFERENT devices of one
 *     process are supported (the kernels' one-time launch state -- > 64 KB dynamic-LDS opt-in, occupancy, CU count -- is
 *     kept per device), each used from one thread at a time;
 *   - there is NO CPU path in this library: with no HIP device every compute
 *     call fails with VDR_ERR_NO_DEVICE.
 */
#ifndef VDR_H_
#define VDR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VDR_ABI_VERSION 8

typedef enum {
  VDR_OK = 0,
  VDR_ERR_INVALID = -1,      /* bad argument / shape / config               */
  VDR_ERR_NO_DEVICE = -2,    /* no gfx950 HIP device visible                */
  VDR_ERR_HIP = -3,          /* a HIP runtime call failed                   */
  VDR_ERR_UNKNOWN_NAME = -4, /* vdr_set_weight: name not part of the config */
  VDR_ERR_WORKSPACE = -5,    /* workspace too small                         */
  VDR_ERR_INCOMPLETE = -6,   /* a weight is missing / vdr_finalize has not run */
  VDR_ERR_UNSUPPORTED = -7   /* config outside what the kernels cover       */
} vdr_status;

typedef enum { VDR_F32 = 0, VDR_BF16 = 1, VDR_F64 = 2, VDR_I16 = 3, VDR_U8 = 4 } vdr_dtype; /* F64 / I16 / U8: pre-processing only */

typedef enum { VDR_ACT_GELU = 0,   /* exact erf GELU: models_archs.py:133, timm/DINOv2 Mlp */
               VDR_ACT_SWIGLU = 1, /* DINOv2 ViT-g SwiGLUFFN (w12 / w3)                   */
               VDR_ACT_QUICK_GELU = 2, /* x sigmoid(1.702 x): OpenAI CLIP vision towers (PubMedCLIP, QuiltNet, PLIP)    */
               VDR_ACT_GELU_TANH = 3   /* 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))): SigLIP ("gelu_pytorch_tanh") */
                                       /* both: weights as VDR_ACT_GELU (mlp.fc1 / mlp.fc2); bf16 path only (fp8 = 1 and  */
                                       /* window > 0 refuse them)                                                         */
} vdr_act;

/* What vdr_forward writes. */
typedef enum {
  VDR_OUT_CLS = 0,         /* [B, D]      final-LN(x)[:,0,:]     (models_archs.py:147 contract)     */
  VDR_OUT_DENSE = 1,       /* [B, n, D]   final-LN(x)[:,P:,:]    (tfds_dense_descriptor.py:130-133); P = has_cls +   */
                           /*             n_register prefix rows: register tokens are discarded with the CLS row   */
  VDR_OUT_PATCH_EMBED = 2, /* [B, n, D]   conv patchify only     (tfds_dense_descriptor.py:128)     */
  VDR_OUT_TOKENS = 3,      /* [B, N, D]   every token after the last block + final LN (if any): N = P + n, rows     */
                           /*             [cls | registers | patches] (transformers last_hidden_state)             */
  VDR_OUT_ENCODER = 4,     /* [B, g, g, C] SAM neck output, channel-LAST (tfds_dense_descriptor.py:123-126   */
                           /*             transposes the reference's [B, C, g, g] to (h, w, C) anyway)     */
  VDR_OUT_POOLED = 5       /* [B, D]      mean over the patch rows (rows P..N-1) of the normalised (or raw)     */
                           /*             stream: vdr_forward_layers only (vdr_forward refuses it)             */
} vdr_out_mode;

/* Geometry of one frozen ViT.  Mirrors the constructor arguments the reference
 * passes to its third-party ViTs (tfds_dense_descriptor.py:87,104) and to
 * nn.TransformerEncoderLayer (models_archs.py:130-135). */
typedef struct {
  int32_t img;        /* native square input side in pixels (224, 336, 896 ...: pos_embed's grid; other sizes: vdr_set_input_size); 0 for a token model */
  int32_t patch;      /* patch side p (14, 16); 0 for a token model                           */
  int32_t in_chans;   /* 3                                                                    */
  int32_t dim;        /* D                                                                    */
  int32_t heads;      /* H ; D / H in {32, 64, 96, 128}; 64 when fp8 = 1 or window > 0        */
  int32_t layers;     /* L                                                                    */
  int32_t mlp_hidden; /* F (GELU: fc1 out; SwiGLU: hidden of w3's input)                      */
  int32_t act;        /* vdr_act                                                              */
  int32_t pre_ln;     /* 1: x += f(LN(x)) + final norm (timm/DINOv2/SAM);                     */
                      /* 0: x = LN(x + f(x)), no final norm (nn.TransformerEncoderLayer)      */
  int32_t layerscale; /* 1: DINOv2 ls1/ls2 gamma                                              */
  int32_t has_cls;    /* 1: a learned cls_token row is prepended                              */
  int32_t has_pos;    /* 1: learned pos_embed [1,N,D] is added                                */
  int32_t input_ln;   /* 1: LayerNorm applied to the assembled tokens before block 0          */
                      /*    (models_archs.py:145; CLIP's pre_layrnorm on an image model,      */
                      /*    which keeps the LayerNorm fold: the input LayerNorm leaves block  */
                      /*    0's row statistics)                                               */
  float ln_eps;       /* 1e-6 timm/DINOv2/SAM, 1e-5 torch default (models_archs.py:136)       */
  int32_t micro_batch;/* images per internal pass (0 = library default: the whole batch, split   */
                      /* evenly over `streams`; with streams == 0 too, the default split below); */
                      /* results do not depend on it                                             */
  int32_t streams;    /* internal HIP streams the micro-batches are spread over; >1 lets kernels of   */
                      /* independent micro-batches overlap, e.g. one part's launch gaps and small     */
                      /* kernels under the other's GEMMs.  1 = the caller's stream only.  0 with an   */
                      /* explicit micro_batch: the same.  0 with micro_batch == 0 = the default split,*/
                      /* decided per call from the batch: the whole batch on the caller's stream, or, */
                      /* where it costs the 8-phase qkv / fc1 GEMMs no extra round of tiles and the   */
                      /* whole batch's last rounds leave 3/4 of a round of the chip idle, two unequal */
                      /* parts on two internal streams (ViT-B/16 at batch 256: 146 + 110; 384 stays   */
                      /* whole; vdr_batch_plan reports it).  Never on a stream that is being */
                      /* captured (a captured forward stays a linear graph), never for fp8 models or  */
                      /* SAM encoders.  streams = 1 forces one stream.  Results do not depend on any  */
                      /* of it: every row is the same bits however the batch is cut                   */
  /* SAM / MedSAM image encoder (segment_anything ImageEncoderViT, tfds_dense_descriptor.py:104,123):   */
  int32_t window;     /* > 0: windowed attention of this side (14) with decomposed relative position   */
                      /* bias in every block; needs has_cls = 0, has_pos = 1, pre_ln = 1               */
  int32_t global_mask;/* bit i set: block i attends over the whole grid (SAM ViT-B: 2,5,8,11 = 0x924)  */
  int32_t neck_chans; /* output channels of the conv neck (256); 1x1 conv, LN2d, 3x3 conv, LN2d        */
                      /* window in {4, 7, 10, 14}.  img: any multiple of patch; with global blocks the     */
                      /* grid side img / patch is at most 64 (VDR_ERR_UNSUPPORTED beyond).  The input size */
                      /* of a SAM encoder is a load-time property, as ImageEncoderViT(img_size=...): a     */
                      /* checkpoint learned at another size loads through vdr_set_weight (below)           */
  /* BASELINE config 5 ("fp8 weights (CDNA4 fp8 MFMA)"): */
  int32_t fp8;        /* 1: the qkv / fc1 (w12) / fc2 (w3) weights are kept as MX-fp8 (OCP e4m3 + e8m0 scale per 32 K    */
                      /* elements) and run on v_mfma_scale_f32_32x32x64_f8f6f4 with MX-fp8 activations; the            */
                      /* out-projection, attention and the residual stream stay bf16; pre_ln only; 0 or 1             */
  int32_t no_ln_fold; /* 0 (default): pre-LN image models fold norm1 / norm2 into the qkv / fc1 GEMMs (the producers of    */
                      /* the residual stream leave row statistics, gamma goes into the weights: no LayerNorm pass);     */
                      /* 1: keep the explicit LayerNorm kernel (numerics A/B, tests)                                    */
  int32_t full_last_block; /* 0 (default): with out_mode VDR_OUT_CLS a pre-LN model runs the out-projection, norm2 and */
                      /* MLP of its LAST block on the CLS rows only -- after the last attention every operation is      */
                      /* row-wise and x[:, 0] is all `model(x) -> (logits, cls)` (models_archs.py:24-29) returns; the   */
                      /* features are bitwise those of the full block.  1: every row (A/B, tests, bench.py              */
                      /* --full-last-block).  Other out_modes and post-LN models always run every row.                  */
  int32_t fp8_cls_bf16; /* fp8 = 1, models with a CLS token: 1 = the MLP (norm2, fc1 / w12, activation, fc2 / w3, residual) of the     */
                      /* CLS ROWS -- one row in ntok per image, the rows the [B, D] CLS feature of models_archs.py:147 is made  */
                      /* of -- runs on the bf16 weights (kept beside the MX-fp8 copies), on a side stream under the fp8 GEMMs of  */
                      /* the other rows; every other row and the qkv projection stay MX-fp8.  Why: a CLS row is carried by     */
                      /* its OWN MLP chain; when the other tokens hold massive-activation channels (DINOv2-g checkpoints) the   */
                      /* attention adds little to it and nothing averages the MX-fp8 rounding of that chain out: row cosine to  */
                      /* fp32 0.989 at 4 blocks / 0.919 at 40 in the stress case of tests/test_model_gpu.py, 0.9986 / 0.9886    */
                      /* with this switch (tools/fp8_outlier_analysis.py, profiles/r04_fp8_outlier_analysis.txt).  0: every row */
                      /* MX-fp8 (stated gate of the fp8 path: row cosine >= 0.99 against fp32 on ordinary weights; under        */
                      /* injected massive-activation channels the CLS rows are gated at 0.985 -- a stated deviation).           */
  int32_t resid_fp32; /* 1 (bf16 path of pre-LN image models; ignored with fp8 = 1, SAM windows and token models): the residual    */
                      /* stream has an fp32 master copy -- the out-projection / fc2 epilogues read it, add in fp32, write it back */
                      /* and write the bf16 copy the next GEMM multiplies; LayerNorm and the final norm read the fp32 copy.  The  */
                      /* reference computes in fp32 throughout (tfds_dense_descriptor.py:123); with the stream stored as bf16      */
                      /* (0, default) its rounding accumulates over the blocks: rel-L2 of the features to fp32 arithmetic 9e-3 /     */
                      /* 1.2e-2 / 1.7e-2 at 12 / 24 / 40 blocks, against 5.8e-3 / 6.6e-3 / 1.0e-2 with this switch                 */
                      /* (tools/resid_precision.py; SURVEY 8d states 1e-2).  Costs 8 more bytes per element of HBM traffic in     */
                      /* the out-projection and fc2 launches.                                                                     */
  int32_t ln_fin_fused; /* LayerNorm fold: where the (sum, sumsq) partials a residual GEMM leaves become (mean, rstd) for a   */
                      /* consumer that reads finalised statistics (large launches).  0 (default): a small ln_finalize launch  */
                      /* between the out-projection / fc2 and the qkv / fc1; 1: inside the residual GEMM -- the workgroup     */
                      /* that adds the last partial to a block of rows finalises the block (ring4 tile variants), no launch.  */
                      /* Same arithmetic: the features are bitwise equal.  Measured equal in time too (ViT-B batch 256: 8.73  */
                      /* vs 8.71-8.74 ms; ViT-L/14@336 batch 64: 25.96 vs 25.99 ms): the counter's round trip at the end of   */
                      /* every tile costs the residual GEMMs what the 23 launches cost, so the simpler form is the default.   */
                      /* (The counters live in the handle, like its internal streams: one forward at a time per handle.)      */
} vdr_config;

/* Geometry that came after vdr_config was frozen (ABI 8 pins its 100 bytes): register tokens and DINOv3's rotary position
 * embedding.  Passed beside vdr_config to vdr_create_ext; vdr_create is vdr_create_ext with ext = NULL (no registers, no
 * RoPE).
 *
 * Register tokens (DINOv2-with-registers `dinov2_vit*14_reg`, DINOv3): n_register learned rows "register_tokens"
 * [1, R, D] sit between the CLS row and the patch rows, so an image is N = P + n token rows with P = has_cls + n_register
 * prefix rows: [cls | registers | patches].  pos_embed stays [1, has_cls + n, D]: the CLS row gets its position, the
 * registers get none, the patch rows theirs (DINOv2-with-registers adds pos_embed before it inserts the registers).
 * Every output mode: VDR_OUT_CLS is row 0; VDR_OUT_TOKENS all N rows; VDR_OUT_DENSE, VDR_OUT_POOLED and the DENSE /
 * POOLED outputs of vdr_forward_layers take rows P.. only (x_norm_patchtokens; the registers are discarded); attention
 * maps keep all N key columns and q_rows = 1 is still the CLS row; the CLS-rows-only last block is unchanged.
 * vdr_set_input_size resamples the patch rows as for any ViT (vdr_op_interpolate_pos).  Stated deviation: upstream's
 * registers variants resample with antialias = True (another cubic kernel); antialiasing is not reproduced here, so at
 * sizes other than the native one the position table differs from upstream's.
 *
 * rope = 1 (DINOv3, transformers DINOv3ViTModel): no position table (has_pos = 0); in every block, between the qkv GEMM
 * and the attention, q and k of the PATCH rows are rotated per head by vdr_op_rope2d with the tables of
 * vdr_op_rope2d_table for the patch grid in force (rebuilt by vdr_finalize / vdr_set_input_size: the model matches
 * transformers at every size).  Prefix rows and v are not rotated.  Attention maps are computed from the rotated buffer.
 * The launches are booked as VDR_K_ASSEMBLE.  q and k are rounded to bf16 twice (after the GEMM, after the rotation);
 * rotating inside the qkv epilogue would remove one rounding and the pass (the partner column lives in another lane's
 * registers there) -- not done.
 *
 * Refused before the device is touched.  VDR_ERR_UNSUPPORTED: n_register > 0 or rope = 1 together with fp8 = 1, window > 0,
 * patch == 0 or pre_ln = 0; rope = 1 with has_pos = 1; rope = 1 with head dim 96 (the frequency step 4 / 96 is inexact in
 * fp32 and no checkpoint uses it); n_register > 16.  VDR_ERR_INVALID: n_register > 0 without has_cls; n_register < 0; rope
 * not 0 / 1; rope = 1 with a non-finite or <= 1 rope_theta; ext->size smaller than the fields below. */
typedef struct {
  int32_t size;        /* sizeof(vdr_config_ext) of the caller: later fields are appended after the ones known today */
  int32_t n_register;  /* 0..16 register tokens between the CLS row and the patch rows (needs has_cls = 1)       */
  int32_t rope;        /* 0 none | 1 DINOv3 axial 2-D RoPE on q and k of the PATCH rows of every block            */
  float   rope_theta;  /* DINOv3: 100                                                                             */
} vdr_config_ext;

typedef struct vdr_model* vdr_handle;

/* ---- lifecycle ------------------------------------------------------------------------ */

/* ABI version of the loaded library (== VDR_ABI_VERSION it was built with). */
int vdr_abi_version(void);

/* 1 when the library was built with -DVDR_TUNING (tools/: diagnostic `variant` encodings >= 100 and VDR_* environment
 * knobs exist), 0 for the shipped build (no environment dependence, unknown variants are an error). */
int vdr_tuning_build(void);

/* Number of visible gfx950 devices (0 when there is none; never fails). */
int vdr_device_count(void);

/* Replaces: model construction in load_dinov2 / load_medsam
 * (tfds_dense_descriptor.py:70-107) and TransformerNoduleClassifier.__init__
 * (models_archs.py:128-139).  Binds the handle to HIP device `device`. */
int vdr_create(const vdr_config* cfg, int device, vdr_handle* out);
/* The same with the extension struct above (NULL: exactly vdr_create). */
int vdr_create_ext(const vdr_config* cfg, const vdr_config_ext* ext, int device, vdr_handle* out);
void vdr_destroy(vdr_handle h);
const char* vdr_last_error(vdr_handle h);

/* Replaces: load_state_dict (models_archs.py:32-35) / sam_model_registry(path)
 * (tfds_dense_descriptor.py:104).  `name` uses the timm/DINOv2 state_dict keys
 * listed in SURVEY.md §8a ("patch_embed.proj.weight", "cls_token", "pos_embed",
 * "blocks.{i}.norm1.weight", "blocks.{i}.attn.qkv.weight", "blocks.{i}.attn.proj.bias",
 * "blocks.{i}.ls1.gamma", "blocks.{i}.mlp.fc1.weight", "blocks.{i}.mlp.w12.weight",
 * "norm.weight", "input_norm.weight" ...).  `host` points to `numel` contiguous fp32
 * values in HOST memory in the PyTorch layout of that key; the library converts,
 * repacks and uploads (synchronously; this is load time, not the hot path).
 * SAM encoder (window > 0) built at another input size than its checkpoint: "pos_embed" is also taken as
 * [1, g0, g0, D] and "blocks.{i}.attn.rel_pos_h" / "rel_pos_w" of a GLOBAL block as [2 g0' - 1, 64], for any g0, g0' in
 * 1..64; vdr_finalize resamples them to the handle's grid g = img / patch once, on the device, as segment_anything
 * does -- pos_embed by vdr_op_interpolate_pos's arithmetic (bicubic, align_corners = False), the rel-pos tables by
 * vdr_op_interpolate_rel_pos's (get_rel_pos: linear, align_corners = False) -- before the bf16 rel-pos pack.  Tables
 * of the handle's own shape are used as loaded (no resampling step).  Window-block tables are [2 window - 1, 64]
 * whatever the grid.  Every other element-count mismatch is VDR_ERR_INVALID. */
int vdr_set_weight(vdr_handle h, const char* name, const float* host, const int64_t* shape, int ndim);

/* Replaces: the end of load_state_dict / model.eval() (models_archs.py:32-35, tfds_dense_descriptor.py:89,105).
 * Call once after the last vdr_set_weight (and again after any later vdr_set_weight): checks that every weight is
 * set, folds LayerNorm into the consuming linears, builds the packed GEMM layouts / MX-fp8 copies / rel-pos tables.
 * Synchronous (hipMalloc, hipMemcpy, hipDeviceSynchronize): this is load time.  vdr_forward* return
 * VDR_ERR_INCOMPLETE until it has run. */
int vdr_finalize(vdr_handle h);

/* Run an image model at another input size, square or rectangular: DINOv2 / transformers interpolate_pos_encoding,
 * done once per size instead of in every forward.  Load-time class (like vdr_finalize: may allocate and synchronise;
 * not for the hot path).  After it every image entry point of the handle -- vdr_forward, vdr_forward_layers,
 * vdr_forward_attn_maps, vdr_workspace_bytes -- takes images [batch, in_chans, height, width]; n = (height / patch) *
 * (width / patch) patches in (y, x) order, N = n + has_cls + n_register tokens.
 *   has_pos = 1: a device table [N, D] fp32 is built -- the CLS row (when there is one) copied unchanged, the patch rows
 *   resampled from the loaded pos_embed's (img / patch)^2 grid by vdr_op_interpolate_pos -- and the forward reads it
 *   wherever it reads pos_embed.  has_pos = 0: geometry only.  height == width == img selects the loaded table itself:
 *   a handle that went to another size and back gives bitwise the features of one that never moved.  One table is
 *   kept (no cache of sizes); a later vdr_finalize (weights changed) rebuilds it for the size in force.  The hot-path
 *   promise (no allocation, no synchronisation in vdr_forward*) holds at any size.  Workspaces must be sized again
 *   (vdr_workspace_bytes); one sized for a smaller geometry is refused with VDR_ERR_WORKSPACE.
 * Supported: pre-LN image models without windows (plain ViT, DINOv2; every vdr_config switch) and layers == 0
 * patch-embedding models.  bf16 images with p in {8, 16, 32} keep the im2col-free gather at square sizes; rectangular
 * sizes go through im2col.  Not reproduced: DINOv2's older scale_factor + interpolate_offset form and antialiasing
 * (DINOv2-with-registers resamples with antialias = True upstream: vdr_config_ext).  rope = 1: the RoPE tables are rebuilt.
 * VDR_ERR_INVALID, before the handle or a device is touched: height <= 0, width <= 0; then a null handle; then a side
 * that is not a multiple of patch.  VDR_ERR_UNSUPPORTED: SAM / MedSAM (window > 0: its absolute and relative position
 * tables and the window partition are tied to its grid; its size is vdr_config.img, chosen at vdr_create), token models (patch == 0), post-LN models with blocks.
 * VDR_ERR_INCOMPLETE: vdr_finalize has not run. */
int vdr_set_input_size(vdr_handle h, int height, int width);
int vdr_get_input_size(vdr_handle h, int* height, int* width);   /* (img, img) until the first set */

/* Run an image model with its frozen patch convolution at a stride below its kernel -- Conv2d(kernel = patch, stride) --
 * for a finer descriptor grid from the same pixels ("Deep ViT Features as Dense Visual Descriptors", dino-vit-features'
 * ViTExtractor(stride=...)): ViT-B/16 on 512^2 at stride 8 gives 63 x 63 patches.  Load-time class, like
 * vdr_set_input_size (may allocate and synchronise), callable before or after it in any order.  The grid in force is
 *   gh x gw = ((height - patch) / stride + 1) x ((width - patch) / stride + 1)
 * for the input size in force, patch (y, x) covering pixels [y*stride, y*stride + patch) x [x*stride, x*stride + patch);
 * n = gh * gw, N = n + has_cls + n_register in every image entry point (vdr_forward's every out_mode,
 * vdr_forward_layers, vdr_forward_attn_maps' q_rows, POOLED's divisor, vdr_workspace_bytes: the col buffer grows with n).
 * The size rule of vdr_set_input_size (sides multiples of patch) is unchanged and makes (side - patch) % stride == 0.
 *   has_pos = 1: the patch rows of the position table are resampled from the loaded (img / patch)^2 grid to gh x gw by
 *   vdr_op_interpolate_pos' rule (bicubic, align_corners = False, size = (gh, gw), fp64, one rounding), the CLS row is
 *   copied, register tokens get none.  Stated deviation: dino-vit-features resamples with the older scale_factor +
 *   0.1-offset form, which is not reproduced (the deviation vdr_set_input_size states for DINOv2).
 *   stride == patch restores the non-overlapping path (the im2col-free gather included): a handle that went to another
 *   stride and back gives bitwise the features of one that never moved.  stride < patch: the images go through the
 *   overlapping im2col (csrc/patch_stride.hip) into the workspace's col buffer, the patch GEMM reads it unchanged.
 * The hot-path promise (no allocation, no synchronisation in vdr_forward*) holds at any stride.
 * Supported: what vdr_set_input_size supports (pre-LN image models without windows, every vdr_config switch, layers == 0
 * patch-embedding models, CLIP / SigLIP towers, register tokens).
 * VDR_ERR_INVALID, before the handle or a device is touched: stride <= 0; then a null handle; then stride > patch or
 * patch % stride != 0.  VDR_ERR_UNSUPPORTED: SAM / MedSAM (window > 0), token models (patch == 0), post-LN models with
 * blocks, rope = 1 (DINOv3's patch coordinates have no upstream definition for overlapping patches to check against).
 * VDR_ERR_INCOMPLETE: vdr_finalize has not run.  A workspace sized for a smaller geometry: VDR_ERR_WORKSPACE. */
int vdr_set_patch_stride(vdr_handle h, int stride);
int vdr_get_patch_stride(vdr_handle h, int* stride);   /* patch until the first set */

/* Number of weight tensors the config expects, and the i-th expected name. */
int vdr_num_weights(vdr_handle h);
const char* vdr_weight_name(vdr_handle h, int i);

/* ---- the hot path ----------------------------------------------------------------------- */

/* Bytes of device workspace vdr_forward / vdr_forward_tokens need for `batch`
 * images (token models: `batch` sequences of `seq` tokens, seq ignored otherwise).
 * The workspace contract, of every entry point that takes (workspace, workspace_bytes) -- vdr_forward, vdr_forward_layers,
 * vdr_forward_attn_maps, vdr_forward_facets, vdr_forward_tokens, vdr_forward_tokens_varlen:
 *   - the contents of `workspace` on entry are irrelevant: any bits, NaN under every element type included, give the
 *     same outputs bit for bit (nothing is read before the call has written it);
 *   - the call reads and writes device memory only inside [workspace, workspace + vdr_workspace_bytes), its inputs,
 *     its outputs and the handle's own weights; the padding rows its kernels read lie inside that range;
 *   - the contents on return are unspecified, and nothing is kept in it between calls;
 *   - workspace_bytes below vdr_workspace_bytes: VDR_ERR_WORKSPACE, and neither the workspace nor any output has been
 *     written.
 * tests/test_workspace_contract_gpu.py holds every kind of forward to this between canary guards. */
int vdr_workspace_bytes(vdr_handle h, int batch, int seq, size_t* out);

/* How a forward of `batch` images (token models: sequences of `seq` tokens) is cut into micro-batches: `parts` passes of
 * `micro_batch` images, the last one the rest, pass k on internal stream k % streams (streams == 1: the caller's stream).
 * It is what vdr_config.micro_batch / streams ask for; with both 0 it is the library's default split (vdr_config.streams):
 * (batch, 1, 1), or two parts on two streams.  On a stream that is being captured the default is always (batch, 1, 1).
 * vdr_workspace_bytes covers the plan reported here and the captured form. */
int vdr_batch_plan(vdr_handle h, int batch, int seq, int32_t* micro_batch, int32_t* parts, int32_t* streams);

/* Replaces: model.image_encoder(x) / model.patch_embed(x)
 * (tfds_dense_descriptor.py:123,128) followed by the CLS / patch-token slice
 * (models_archs.py:147; tfds_dense_descriptor.py:130-133), batched.
 *   images : device, NCHW [batch, in_chans, img, img] ([.., height, width] after vdr_set_input_size), dtype in_dtype, values as the
 *            reference feeds them (raw [0,1]; no mean/std normalisation is applied)
 *   out    : device, shape by out_mode, dtype out_dtype, C-contiguous, row b = image b */
int vdr_forward(vdr_handle h, const void* images, int in_dtype, int batch, void* out, int out_mode,
                int out_dtype, void* workspace, size_t workspace_bytes, void* stream);

/* Features from inside the encoder, several per forward: DINOv2 get_intermediate_layers(x, n, reshape,
 * return_class_token, norm) and the linear-probe descriptor of create_linear_input (CLS rows of the last blocks and
 * the mean of the last block's normalised patch tokens, concatenated: [B, 5*D] for 4 blocks).  One output: */
typedef struct {
  int32_t layer;     /* block index 0 .. L-1: the residual stream after that block                                */
  int32_t out_mode;  /* VDR_OUT_CLS [B, D] | VDR_OUT_DENSE [B, n, D] | VDR_OUT_TOKENS [B, N, D] | VDR_OUT_POOLED [B, D] */
  int32_t out_dtype; /* VDR_F32 | VDR_BF16                                                                        */
  int32_t norm;      /* 1: through the model's final norm (DINOv2 norm=True); 0: the raw stream the next block reads */
  int64_t ld;        /* CLS / POOLED: elements between consecutive images' rows (0 = D, else >= D); DENSE / TOKENS: 0 */
  void* out;         /* device buffer; image b's row(s) start at out + b*ld (CLS/POOLED) or b*rows*D (DENSE/TOKENS)   */
} vdr_layer_out;

/* One forward of a pre-LN image model (plain ViT, DINOv2: LayerScale, SwiGLU, fp8, fp8_cls_bf16, resid_fp32, no_ln_fold,
 * micro_batch, streams) that writes all n_outs outputs, in any order; several may name the same layer.  Blocks past the
 * largest requested layer do not run.  The output of block i is bitwise vdr_forward's on the same weights truncated to
 * i + 1 blocks (norm = 1; CLS / DENSE / TOKENS): it is the same final-LayerNorm launch on the same stream, written after
 * the block's last residual GEMM.  norm = 0 copies the raw stream (its fp32 copy with resid_fp32) with one rounding to
 * out_dtype.  POOLED is the fp32 mean over the n patch rows, in fixed-size chunks and a fixed order (no atomics, the
 * same bits in any batch), rounded once.  When every output of the last block that runs is CLS, that block runs its
 * CLS rows only (vdr_config.full_last_block), as vdr_forward does.  Workspace: vdr_workspace_bytes (unchanged).
 * Refused before the device is touched: SAM (window > 0), token and post-LN models, layers == 0
 * (VDR_ERR_UNSUPPORTED); null pointers, n_outs <= 0, a layer out of range, an unknown mode, dtype or norm flag, CLS on a
 * model without a CLS token, ld in (0, D) or negative, a non-zero ld for DENSE / TOKENS (VDR_ERR_INVALID). */
int vdr_forward_layers(vdr_handle h, const void* images, int in_dtype, int batch, const vdr_layer_out* outs, int n_outs,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Attention maps of any block (DINO get_last_selfattention, output_attentions, the per-head CLS heat map): the
 * normalised softmax(q k^T dh^-0.5) of one block's attention, computed from the block's own qkv activation right after
 * its attention (vdr_op_attention_probs).  One map: */
typedef struct {
  int32_t layer;     /* block 0 .. L-1 whose attention is reported                                  */
  int32_t q_rows;    /* 1 .. N: the first q_rows query rows (1 = the CLS row, N = the full map)      */
  int32_t head_mean; /* 0: [B, H, q_rows, N]; 1: [B, q_rows, N], mean over the heads                 */
  int32_t out_dtype; /* VDR_F32 | VDR_BF16                                                           */
  void* out;         /* device, contiguous; image b's map starts at out + b * (per-image elements)   */
} vdr_attn_map;

/* vdr_forward_layers plus n_maps >= 1 attention maps, in one forward.  The outs have exactly vdr_forward_layers' meaning,
 * checks and bits (n_outs may be 0 with outs NULL).  Blocks past the largest requested layer (outs and maps together) do
 * not run; a last block whose only requests are maps stops after its attention.  Supported models, workspace and the
 * VDR_ERR_UNSUPPORTED refusals: those of vdr_forward_layers.  Refused before the device is touched (VDR_ERR_INVALID): null
 * maps, n_maps <= 0, a null out, q_rows outside [1, N], head_mean not 0 / 1, an unknown dtype, a layer out of range.
 * The map launches are booked as VDR_K_FINAL_LN. */
int vdr_forward_attn_maps(vdr_handle h, const void* images, int in_dtype, int batch, const vdr_layer_out* outs, int n_outs,
                          const vdr_attn_map* maps, int n_maps, void* workspace, size_t workspace_bytes, void* stream);

/* Facet descriptors ("Deep ViT Features as Dense Visual Descriptors", ViTExtractor.extract_descriptors(x, layer, facet,
 * bin, include_cls)): the keys, queries or values of one block's attention, or the residual stream after it, optionally
 * log-binned.  With P prefix rows (CLS + registers), n = gh * gw patch rows, N = P + n:
 *   QUERY | KEY | VALUE of block i: the output of its qkv linear, bias included, heads concatenated -- columns [0, D),
 *     [D, 2D), [2D, 3D) of the [B*N, 3D] bf16 activation the attention kernels read -- BEFORE the 2-D RoPE rotation of a
 *     vdr_config_ext.rope model (what a forward hook on attn.qkv sees) and before any dh^-0.5 scale.
 *   TOKEN of block i: the raw residual stream after it, bitwise a vdr_layer_out with norm = 0 in VDR_OUT_DENSE
 *     (all_rows = 0) or VDR_OUT_TOKENS (all_rows = 1) mode at the same dtype.
 *   hierarchy = 0: [B, n, D] (all_rows = 1: [B, N, D], rows as VDR_OUT_TOKENS orders them), one rounding to out_dtype.
 *   hierarchy = h in 1..3: vdr_op_log_bin of the n patch rows on the gh x gw grid, [B, n, (1 + 8h) * D]; all_rows must be 0. */
enum { VDR_FACET_TOKEN = 0, VDR_FACET_QUERY = 1, VDR_FACET_KEY = 2, VDR_FACET_VALUE = 3 };
typedef struct {
  int32_t layer;     /* block 0 .. L-1                                                               */
  int32_t facet;     /* VDR_FACET_TOKEN | QUERY | KEY | VALUE                                        */
  int32_t hierarchy; /* 0: no binning; 1..3: log-binned                                              */
  int32_t all_rows;  /* 0: the n patch rows; 1: all N rows (hierarchy must be 0)                     */
  int32_t out_dtype; /* VDR_F32 | VDR_BF16                                                           */
  void* out;         /* device, contiguous; image b's rows start at out + b * (per-image elements)   */
} vdr_facet_out;

/* vdr_forward_attn_maps plus n_facets >= 1 facets, in one forward.  outs and maps keep exactly their meaning, checks and
 * bits; either may be empty (NULL, 0).  Facets may name any blocks in any order, several per block.  q / k / v facets of
 * block i are written right after its qkv GEMM, before the rotation and the attention: unbinned as a strided row gather,
 * binned by the log-bin kernel reading the qkv activation in place, its level means in the (then dead) fc1 activation
 * buffer.  A TOKEN facet is written where the block's outs are.  Blocks past the largest requested layer do not run; a
 * last block whose only requests are q / k / v facets stops after its qkv GEMM (with maps: after its attention); a TOKEN
 * facet needs every row of its block, so the CLS-rows-only last block does not apply then.  Facet launches are booked as
 * VDR_K_FINAL_LN.  Supported models, workspace and VDR_ERR_UNSUPPORTED refusals: those of vdr_forward_layers, plus a
 * hierarchy whose level means ((h - 1) * micro-batch * n * D fp32) do not fit the fc1 activation buffer, or with D % 8 != 0
 * (both refused before anything is launched or written).  fp8 handles are
 * allowed: their qkv activation is the same bf16 [q | k | v] image the attention reads (the MX GEMM writes bf16 there).
 * Refused before the device is touched (VDR_ERR_INVALID): null facets, n_facets <= 0, a null out, a layer out of range,
 * an unknown facet or dtype, hierarchy outside 0..3, all_rows not 0 / 1 or set together with a hierarchy. */
int vdr_forward_facets(vdr_handle h, const void* images, int in_dtype, int batch, const vdr_layer_out* outs, int n_outs,
                       const vdr_attn_map* maps, int n_maps, const vdr_facet_out* facets, int n_facets, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Replaces: TransformerNoduleClassifier.forward up to x[:,0,:]
 * (models_archs.py:141-147): tokens [batch, seq, D] fp32/bf16 on device ->
 * [cls ; tokens] -> (input LN) -> L blocks -> out by out_mode
 * (VDR_OUT_CLS -> [batch, D]; VDR_OUT_TOKENS -> [batch, seq+has_cls, D]). */
int vdr_forward_tokens(vdr_handle h, const void* tokens, int in_dtype, int batch, int seq, void* out,
                       int out_mode, int out_dtype, void* workspace, size_t workspace_bytes,
                       void* stream);

/* Variable-length token sequences: the reference feeds one patient's masked-voxel sequence at a
 * time (batch_size 1, train_models.py:143-182 / conf parameters_models.yaml); here `batch` sequences padded to
 * max_seq go through one call.  seq_lens: device int32 [batch], 1 <= seq_lens[b] <= max_seq; rows past a
 * sequence's length may hold anything finite — attention masks them as keys, and the rows of a sequence never
 * mix with another's.  Outputs as vdr_forward_tokens (VDR_OUT_CLS is what models_archs.py:147 returns); rows of
 * VDR_OUT_TOKENS / DENSE past a sequence's length are undefined. */
int vdr_forward_tokens_varlen(vdr_handle h, const void* tokens, int in_dtype, int batch, int max_seq,
                              const int32_t* seq_lens, void* out, int out_mode, int out_dtype, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ---- single operators (the torch ops the reference invokes underneath R2/R3) ------------ */
/* Exposed so that each HIP kernel is parity-tested against its torch op through
 * this ABI (tests/test_ops_gpu.py).  All pointers are device pointers. */

/* F.layer_norm(x, (D,), gamma, beta, eps)  — nn.LayerNorm at models_archs.py:136,145 and
 * norm1/norm2/norm of the ViT blocks.  x [rows, D] in_dtype -> y [rows, D] out_dtype;
 * gamma/beta fp32 [D].  rows >= 1 (else VDR_ERR_INVALID); D a positive multiple of 4, at most 2048 (else
 * VDR_ERR_UNSUPPORTED).  Alignment (a lane moves 4 elements per access): x and y to 4 elements of their type -- 8 bytes
 * for bf16, 16 for fp32 -- gamma and beta to 16 bytes; anything else is VDR_ERR_INVALID before the device is touched. */
int vdr_op_layernorm(const void* x, int in_dtype, void* y, int out_dtype, const float* gamma,
                     const float* beta, int64_t rows, int D, float eps, void* stream);

/* epilogues of vdr_op_linear */
typedef enum {
  VDR_EPI_BIAS = 0,      /* y = xW^T + b                      F.linear                          */
  VDR_EPI_BIAS_GELU = 1, /* y = gelu_erf(xW^T + b)            linear1 + activation (a9).  Deviation from torch: a NaN   */
                         /*   input gives -3e-8, not NaN (the device form is max(x,0) - a 2^Q(a) on v_min / v_max, which   */
                         /*   return their non-NaN operand; csrc/vdr_dev.h).  Inside a block the residual stream carries   */
                         /*   the NaN row on regardless; the classifier heads hand non-finite rows on themselves.          */
  VDR_EPI_BIAS_RESID = 2,/* y = resid + gamma*(xW^T + b)      out_proj / linear2 + residual     */
  VDR_EPI_SWIGLU = 3,    /* y[:, :N/2] = silu(a)*b, (a,b) = split(xW^T + b)  DINOv2 SwiGLUFFN   */
  /* (4 .. 7 are internal to the library) */
  VDR_EPI_BIAS_QUICK_GELU = 8, /* y = a sigmoid(1.702 a), a = xW^T + b            CLIP MLP (QuickGELU)                    */
  VDR_EPI_BIAS_GELU_TANH = 9   /* y = gelu(a, approximate="tanh")                 SigLIP MLP ("gelu_pytorch_tanh")        */
                         /*   both as a / (1 + 2^(-t log2 e)), t = 1.702 a or 2 sqrt(2/pi) (a + 0.044715 a^3), in fp32 on */
                         /*   v_exp_f32 / v_rcp_f32 (csrc/vdr_dev.h): within a few fp32 ulp of the exact function before  */
                         /*   the one bf16 rounding.  NaN propagates; -inf gives NaN (torch's tanh form: -0).  Accepted by  */
                         /*   vdr_op_linear, vdr_op_linear_packed and vdr_op_linear_ln_fold wherever VDR_EPI_BIAS_GELU is  */
                         /*   (every tile variant, the 8-phase kernel included); vdr_op_linear_mx does not carry them      */
} vdr_epilogue;

/* F.linear(x, W, b) (+ fused epilogue) — nn.Linear inside nn.MultiheadAttention /
 * TransformerEncoderLayer (models_archs.py:130-135), attn.qkv / attn.proj / mlp.fc1 / mlp.fc2.
 *   x [M, K] bf16, W [N, K] bf16 (PyTorch layout), bias fp32 [N] or NULL,
 *   resid [M, N] bf16 (EPI_BIAS_RESID; may alias y), gamma fp32 [N] or NULL (LayerScale),
 *   y [M, N] bf16 (EPI_SWIGLU: [M, N/2]).  K % 64 == 0, N % 8 == 0.
 *   `variant` selects the tile configuration (0 = library default).
 *   Alignment: x, W, bias, resid, gamma and y each to 16 bytes (16-byte operand loads of x and W, f32x4 loads of bias and
 *   gamma, bf16x8 loads of resid and stores of y; with K % 64 == 0 and N % 8 == 0 every row then is).  A pointer off
 *   that boundary is VDR_ERR_INVALID before the device is touched; the same for vdr_op_linear_packed. */
int vdr_op_linear(const void* x, const void* W, const float* bias, const void* resid,
                  const float* gamma, void* y, int64_t M, int N, int K, int epilogue, int variant,
                  void* stream);
/* The same with W in the library's packed weight layout — what vdr_finalize builds for every nn.Linear weight of a
 * model: [N/2][K/32][2][32] bf16, so that a 128-byte line holds one 32-deep K block of two neighbouring rows and the
 * operand loader of the GEMM touches whole lines.  vdr_op_pack_linear_weight converts W [N, K] bf16 (PyTorch layout)
 * into `packed` (N*K bf16, device); N even, K % 32 == 0.  Results are bitwise those of vdr_op_linear. */
int vdr_op_pack_linear_weight(const void* W, int N, int K, void* packed, void* stream);
int vdr_op_linear_packed(const void* x, const void* Wp, const float* bias, const void* resid,
                         const float* gamma, void* y, int64_t M, int N, int K, int epilogue, int variant,
                         void* stream);

/* ---- the LayerNorm fold (pre-LN image models; csrc/gemm_kernels.h) ---------------------------------
 * The forward never materialises norm1 / norm2: the residual GEMMs leave per-row (sum, sum of squares) partials of the
 * bf16 rows they store, one slot per 64-column group; these become (mean, rstd); the consuming GEMM runs on the folded
 * weight and applies y = rstd * (x.W'^T - mean * colsum) + tbias in its epilogue.  These entry points run the forward's
 * own arithmetic and launch code on caller buffers.  All but vdr_ln_fold_weights take device pointers.
 *
 * Host only: the fold of one linear (W [N, K], b [N]) behind LayerNorm (gamma, beta [K]), fp32 host arrays in, host
 * arrays out: wf [N, K] bf16 bits = bf16(gamma . W), colsum[n] = float(sum_k wf[n][k]), tbias[n] = float(sum_k beta[k]
 * W[n][k] + b[n]).  swiglu = 1: W / b are mlp.w12 in PyTorch order ([x1 | x2]); the outputs come in the gate-pair order
 * the SwiGLU epilogue reads (ops.pack_w12).  N % 64 == 0 then. */
int vdr_ln_fold_weights(const float* W, const float* b, const float* gamma, const float* beta, int N, int K, int swiglu,
                        uint16_t* wf, float* colsum, float* tbias);
/* Producer: vdr_op_linear with EPI_BIAS_RESID (y = resid + gamma*(xW^T + b), y may alias resid) that also writes the
 * partials of y's bf16 rows to part [N/64][part_stride][2] fp32.  resid32 / y32 non-NULL: the fp32 residual stream
 * (read from resid32 [M, N], the fp32 sum written to y32, y = its bf16 rounding; the partials are of y); resid may
 * then be NULL.  stats non-NULL: the last workgroup of every 64-row block also finalises (mean, rstd) into stats [M][2],
 * counting with `counters` (uint32, at least ceil(M / 64), zeroed; left zeroed): ring4 variants 26..29 only.
 * variant 22..29, N % 64 == 0, K % 64 == 0, part_stride >= M. */
int vdr_op_linear_ln_stats(const void* x, const void* W, const float* bias, const void* resid, const float* gamma, void* y,
                           const float* resid32, float* y32, int64_t M, int N, int K, int variant, float* part,
                           int64_t part_stride, float* stats, uint32_t* counters, float eps, void* stream);
/* Finaliser: part [D/64][part_stride][2] -> stats [rows][2] (mean, rstd), var = E[x^2] - mean^2 in double. */
int vdr_op_ln_finalize(const float* part, int64_t part_stride, int64_t rows, int D, float eps, float* stats, void* stream);
/* Consumer: y = epi(rstd * (x.Wf^T - mean * colsum) + tbias) for x [M, K] bf16 (the residual stream), Wf [N, K] bf16,
 * colsum / tbias fp32 [N].  Exactly one of stats [M][2] (finalised) and part (the producer's partials, finalised
 * inside the GEMM: variants 22-24 and 26-28, K <= 1024).  epilogue VDR_EPI_BIAS, _GELU or _SWIGLU (Wf / colsum / tbias
 * in gate-pair order, y [M, N/2]); variant 22..29 or 31 (the 8-phase kernel, where eligible).  x_rows: rows of x and of
 * stats that are readable (>= M; 0 = M): variant 31 takes a ragged M only when they cover M rounded up to 256. */
int vdr_op_linear_ln_fold(const void* x, const void* Wf, const float* colsum, const float* tbias, const float* stats,
                          const float* part, int64_t part_stride, void* y, int64_t M, int N, int K, int64_t x_rows, float eps,
                          int epilogue, int variant, void* stream);

/* ---- MX-fp8 operators (BASELINE config 5: "DINOv2 ViT-g/14 fp8 weights (CDNA4 fp8 MFMA)") ----------
 * An MX tensor X[rows, K] is an OCP e4m3 payload q[rows, K] (one byte per element) plus e8m0 scales, one per
 * 32 consecutive K elements, in the device layout  s[K/32][rows_pad]  (rows_pad = rows rounded up to 256; inside
 * each 64-row group rows are stored as (r, r+32) pairs).  vdr_mx_scale_bytes gives the size of that array.
 * The reference has no fp8 path (fp32 eager everywhere); these replace the same nn.Linear / nn.LayerNorm
 * call sites as vdr_op_linear / vdr_op_layernorm (models_archs.py:130-136, ViT blocks). */
size_t vdr_mx_scale_bytes(int64_t rows, int K);
/* bf16 x [rows, K] -> MX (q, scales).  K % 32 == 0. */
int vdr_op_mx_quantize(const void* x, int64_t rows, int K, void* q, void* scales, void* stream);
/* MX (q, scales) -> fp32 y [rows, K]  (test / inspection helper: value = e4m3(q) * 2^(scale-127)) */
int vdr_op_mx_dequantize(const void* q, const void* scales, int64_t rows, int K, float* y, void* stream);
/* F.layer_norm over bf16 rows with MX output (the operand of the following fp8 linear).  D % 32 == 0. */
int vdr_op_layernorm_mx(const void* x, const float* gamma, const float* beta, float eps, int64_t rows, int D,
                        void* q, void* scales, void* stream);
/* F.linear with MX operands on the block-scaled fp8 MFMA, fp32 accumulate, same epilogues as vdr_op_linear.
 *   xq/xs: MX x [M, K];  wq/ws: MX W [N, K];  y bf16 [M, N] ([M, N/2] for EPI_SWIGLU), or — when yscales is
 *   non-NULL (EPI_BIAS_GELU / EPI_SWIGLU only) — an MX tensor (y = payload, yscales) ready for the next
 *   fp8 linear.  K % 64 == 0, N % 64 == 0.  variant: 0 = 128x256 tile, 1 = 256x256, 2 = 128x128. */
int vdr_op_linear_mx(const void* xq, const void* xs, const void* wq, const void* ws, const float* bias,
                     const void* resid, const float* gamma, void* y, void* yscales, int64_t M, int N, int K,
                     int epilogue, int variant, void* stream);

/* ---- pre/post-processing either side of the encoder --------------------------
 * What the reference does per slice on the CPU with numpy / skimage; all pointers are device pointers. */

/* prepare_image (tfds_dense_descriptor.py:30-48) for a batch of slices: gray2rgb, skimage.transform.resize
 * (order 1, mode 'reflect', anti-aliasing Gaussian when down-scaling, float64 arithmetic), HWC -> CHW; the
 * flips of flip_image (:305-324) are folded in.
 *   src        fp32 (src_dtype VDR_F32) or fp64 (VDR_F64) image(s) with ELEMENT strides (stride_b, stride_y,
 *              stride_x, stride_c): the slices of an (H, W, S[, C]) volume are a batch as they lie
 *   channels   1 (replicated to 3, target side 1024 in the reference) or 3 (target side 896)
 *   flip       0 none, 1 'horizontal' (x reversed), 2 'vertical' (y reversed)
 *   out        [batch, 3, out_side, out_side] fp32 or bf16 (out_dtype)
 *   scratch    device scratch of vdr_prepare_scratch_bytes(...) bytes (0 when nothing is down-scaled) */
size_t vdr_prepare_scratch_bytes(int batch, int h, int w, int channels, int out_side);
int vdr_op_prepare_image(const void* src, int src_dtype, int batch, int h, int w, int channels, int64_t stride_b,
                         int64_t stride_y, int64_t stride_x, int64_t stride_c, int flip, int out_side, void* out,
                         int out_dtype, void* scratch, void* stream);
/* apply_window_ct (tfds_dense_descriptor.py:287-302, windowing_ct :204-237): clip((ct - (L - W/2)) / W, 0, 1).
 *   ct fp32 (VDR_F32) or int16 (VDR_I16), n elements -> out fp32 */
int vdr_op_window_ct(const void* ct, int in_dtype, int64_t n, double width, double level, float* out, void* stream);
/* hu_to_rgb_vectorized (visualization_utils.py:128-186): HU -> uint8 RGB [n, 3].  hu fp32 / int16 / fp64. */
int vdr_op_hu_to_rgb(const void* hu, int in_dtype, int64_t n, void* rgb, void* stream);
/* crop_image / extract_roi (visualization_utils.py:93-125) of channel-last maps:
 *   src fp32 [batch, H, W, C] -> dst fp32 [batch, crop_h, crop_w, C], window origin (y0, x0), fully inside */
int vdr_op_crop_hwc(const float* src, float* dst, int batch, int H, int W, int C, int y0, int x0, int crop_h,
                    int crop_w, void* stream);
/* rotate_image (tfds_dense_descriptor.py:327-350): scipy.ndimage.rotate(vol, angle, axes=(0, 1), reshape=False,
 * mode='nearest') = scipy.ndimage.affine_transform(plane, matrix, offset, order=3, mode='nearest', prefilter=True)
 * on every (H, W) plane of the volume; float64 arithmetic in SciPy's operation order (bit-identical results).
 *   src      [h, w, planes] (planes = slices [x channels], fastest) fp64 (VDR_F64), fp32 (VDR_F32) or a boolean mask
 *            as bytes 0 / 1 (VDR_U8); out has the same shape and dtype
 *   matrix   2 x 2 row-major, offset 2: input coordinate = matrix . output index + offset (SciPy's convention;
 *            rotate() passes [[cos, sin], [-sin, cos]] and in_center - matrix . out_center)
 *   clip01   1: clip the float result to [0, 1] (the np.clip of rotate_image); masks: out = (unsigned char) t,
 *            SciPy's store into a boolean output, so `out > 0` is rotate_image's mask
 *   scratch  vdr_affine_cubic_scratch_bytes(h, w, planes) bytes: the edge-padded float64 spline coefficients */
size_t vdr_affine_cubic_scratch_bytes(int h, int w, int64_t planes);
int vdr_op_affine_cubic(const void* src, int dtype, int h, int w, int64_t planes, const double* matrix,
                        const double* offset, void* out, int clip01, void* scratch, void* stream);
/* Stage-C input sequence (train_models.py:143-182 'transformer' branch + positional_encoding_3d :30-44):
 * out[r, :] = feat[index[r], :] + PE(x_r, y_r, z_r) / 4, the masked voxels of an (h, w, S) feature volume with their
 * 3-D sinusoidal position code.
 *   feat   fp32 [positions, D], positions in (h, w, S) order;  index int64 [n] positions kept (ascending)
 *   xyz    fp64 [3][n] coordinates of the kept voxels;  expo fp64 [D / 6] = scale^(6 i / D)
 *   out    [n, D] fp32 (VDR_F32), bf16 (VDR_BF16) or fp64 (VDR_F64, what numpy produces) */
int vdr_op_voxel_sequence(const float* feat, const int64_t* index, const double* xyz, const double* expo, int64_t n,
                          int D, void* out, int out_dtype, void* stream);

/* F.scaled_dot_product_attention over a packed qkv activation — the core of
 * nn.MultiheadAttention (models_archs.py:130) / Attention.forward of the ViTs.  Head dim 64; any head dim of
 * vdr_config.heads: vdr_op_attention_hd.
 *   qkv [batch*seq, 3*H*64] bf16, row = token, columns [q | k | v] each [H, 64]
 *   out [batch*seq, H*64] bf16;  softmax(q k^T / 8) v per (batch, head), no mask.
 *   variant: 0 = library choice; 1 = chunked (online softmax over 128-key chunks), 2 = persistent kernel without,
 *   4 = with its loader wave (sequences of 129..224 tokens), 3 = one workgroup per (batch, head).  All variants
 *   produce the same bits for sequences that fit one chunk.
 *   batch, seq or heads <= 0: VDR_ERR_INVALID (also vdr_op_attention_hd and vdr_op_attention_varlen). */
int vdr_op_attention(const void* qkv, void* out, int batch, int seq, int heads, int variant,
                     void* stream);

/* The same at head dim dh = head_dim in {32, 64, 96, 128}:
 *   qkv [batch*seq, 3*H*dh] bf16, columns [q | k | v] each [H, dh];  out [batch*seq, H*dh] bf16;
 *   softmax(q k^T dh^-0.5) v per (batch, head), no mask, any seq >= 1.
 *   head_dim 64 is vdr_op_attention (same kernels, same bits, same variants).  32 / 96 / 128 run one kernel (online
 *   softmax over key chunks) whatever the variant (0..4); a (batch entry, head)'s output does not depend on batch.
 *   Any other head_dim: VDR_ERR_UNSUPPORTED. */
int vdr_op_attention_hd(const void* qkv, void* out, int batch, int seq, int heads, int head_dim, int variant,
                        void* stream);

/* The same with per-sequence lengths (the masking vdr_forward_tokens_varlen runs): batch entry b attends over its
 * first len_b = min(seq, lens[b] + len_add) rows only, as keys; rows past len_b are padding.
 *   lens  device int32 [batch]; every lens[b] + len_add >= 1
 *   Rows < len_b of the output do not depend on the padding rows' contents (any bits, NaN and Inf included) nor on
 *   seq; rows >= len_b are undefined.  With lengths only the one-shot (3) and online (1) kernels run: variants 0, 2
 *   and 4 take the one-shot kernel at seq <= 288.  head_dim as vdr_op_attention_hd. */
int vdr_op_attention_varlen(const void* qkv, void* out, int batch, int seq, int heads, int head_dim,
                            const int32_t* lens, int len_add, int variant, void* stream);

/* The attention map of the same qkv: P = softmax(q k^T dh^-0.5) of the first q_rows query rows of every (batch entry,
 * head), normalised, fp32 or bf16 (out_dtype; bf16 is one rounding of the fp32 value).
 *   out [batch, H, q_rows, seq] (head_mean = 0) or [batch, q_rows, seq] (head_mean = 1: the mean over the heads)
 *   s = q.k in fp32 on the bf16 MFMA, t = s * c (c the fp32 dh^-0.5 log2(e) of the attention kernels), m = max t,
 *   e = exp2(t - m), l = sum e (fp32), p = e * (1 / l) with one correctly rounded division per row; head_mean:
 *   (sum of p over the heads in head order, fp32) * RN(1 / H).  No atomics: a row's bits depend neither on batch nor
 *   on the launch.  head_dim in {32, 64, 96, 128} (else VDR_ERR_UNSUPPORTED), 1 <= q_rows <= seq. */
int vdr_op_attention_probs(const void* qkv, void* out, int batch, int seq, int heads, int head_dim, int q_rows,
                           int head_mean, int out_dtype, void* stream);

/* One-query attention pooling -- the attention of SigLIP's pooling head (transformers
 * SiglipMultiheadAttentionPoolingHead: nn.MultiheadAttention with one learned probe as the only query):
 *   out[b, h*dh + d] = sum_j softmax_j(q_h . k[b, j, h] dh^-0.5) v[b, j, h, d]  over the n tokens j of image b
 *   q    device fp32 [heads * head_dim]: the probe after the q projection (and its bias), the same for every image; the
 *        dh^-0.5 scale is applied here
 *   kv   device bf16, row b * n + j = token j of image b, ldkv elements apart: columns [0, H dh) k, [H dh, 2 H dh) v (one
 *        GEMM with the k and v rows of in_proj_weight); 16-byte aligned, ldkv % 8 == 0, ldkv >= 2 * heads * head_dim
 *   out  device bf16 [batch, heads * head_dim]
 * fp32 arithmetic: the maximum is subtracted, sum p v and sum p are accumulated unnormalised and divided once, one
 * rounding to bf16.  Each k / v byte is read once (16-byte loads).  The keys are split over the waves of a workgroup and
 * combined through LDS in a fixed order: no atomics, a row's bits do not depend on batch.
 * Refused before the device is touched: head_dim not in {32, 64, 96, 128} (VDR_ERR_UNSUPPORTED); null pointers,
 * batch <= 0, heads <= 0, n < 1, a bad ldkv or alignment (VDR_ERR_INVALID). */
int vdr_op_attention_pool(const float* q, const void* kv, int64_t ldkv, void* out, int batch, int n, int heads, int head_dim,
                          void* stream);

/* ---- mask decoder ops: the kernels of SAM's box-prompt mask decoder (csrc/mask_decoder.hip; the decoder object below
 * composes them with the GEMM and LayerNorm of the forward).  A "problem" is one (image, box) pair.  All three are compiled without floating-point
 * contraction: every multiply and add below is rounded once unless written fma().
 *
 * Cross attention with a handful of rows on one side (segment_anything Attention inside TwoWayAttentionBlock):
 *   out[p, i, h*dh + d] = sum_j softmax_j(Q[p,i,h] . K[p,j,h] dh^-0.5) v[p, j, h*dh + d]
 *   Q[p,i,c] = float(q[p,i,c]) + q_add[i,c],  K[p,j,c] = float(k[p,j,c]) + k_add[j,c]   (one fp32 addition; no table: the float)
 *   q    device bf16, row p * tq + i, ldq elements apart;  k, v  device bf16, row p * tk + j, ldk / ldv apart;  out  bf16, row
 *        p * tq + i, ldo apart.  Each is read in place: a column slice of a wider buffer (a stacked projection) is fine.
 *   q_add / k_add  device fp32 [tq, heads*dh] / [tk, heads*dh], dense, shared by every problem, or NULL: the positional-encoding
 *        term pe W^T + b of a projection whose input is x + pe.
 * head_dim 16 or 32, heads * head_dim <= 256, one of tq, tk at most 16.  s = the fma chain over d ascending from 0 (tk <= 16) or
 * over the 8 columns of each 16-byte chunk followed by the chunks added in a tree (tk > 16); t = s * fp32(dh^-0.5 log2 e);
 * p = 2^(t - m) on v_exp_f32.
 *   tk <= 16 ("few keys"): K and v of the problem are held in LDS as fp32, one lane per (query row, head); m = max_j t_j,
 *        L = p_0 + p_1 + ..., A_d = fma(p_j, v_jd, A_d) for j ascending, out = bf16(A_d / L): one IEEE division, one rounding.
 *   tk > 16, tq <= 16 ("few queries"): one workgroup of 4 waves per (problem, head); key j goes to wave (j / KPW) % 4, slot
 *        j % KPW (KPW = 512 / dh keys per wave and step), every (wave, slot) runs an online softmax per query (running maximum
 *        m, l = fma(l, 2^(m - m'), p), acc likewise); the slots of a wave are rescaled to the wave's maximum and added in a
 *        butterfly tree, the 4 waves in ascending order through LDS; out = bf16(A / L).  Every k / v byte is read once, 16 bytes
 *        per lane.  Any summation order obeys |A_d - exact| <= gamma(tk + 2) sum_j p_j |v_jd| (tests/sam_decoder_ref.py).
 * No atomics; which lane sums what depends on (tq, tk, dh) only, so a problem's bits do not depend on `problems` or its position.
 * Refused before the device is touched: null q / k / v / out, non-positive sizes, problems > 65535, a leading dimension below
 * heads*dh or no multiple of 8, a pointer off 16 bytes (VDR_ERR_INVALID); head_dim not 16 or 32, heads*dh > 256, tq and tk both
 * above 16 (VDR_ERR_UNSUPPORTED). */
int vdr_op_cross_attention(const void* q, int64_t ldq, const float* q_add, const void* k, int64_t ldk, const float* k_add,
                           const void* v, int64_t ldv, void* out, int64_t ldo, int problems, int tq, int tk, int heads,
                           int head_dim, void* stream);

/* The token-side linear of the mask decoder (M = a few rows per problem, where a tile GEMM would be one ragged tile):
 *   y[r, n] = [max(., 0)](sum_k X[r,k] W[g][n,k] + bias[g][n]) [+ float(resid[r, n])],   g = r % groups
 *   X[r,k] = float(x[r,k]), or with x_add float(bf16(float(x[r,k]) + float(x_add[r,k])))  (torch's bf16 `x + pe`)
 *   x, x_add, resid  device bf16, rows ldx / ldxa / ldr elements apart (x_add, resid may be NULL; resid may be y);
 *   W  device bf16 [groups, N, K] (PyTorch layout per group), 16-byte aligned; bias fp32 [groups, N] or NULL;
 *   y  bf16 or fp32 (out_dtype), rows ldy apart.
 * The sum: 16 partial sums, partial q over the 8-element chunks q, q + 16, q + 32, .. of the row (k = 8 chunk .. 8 chunk + 7), each
 * one fp32 fma chain in ascending k from 0; the partials added in ascending q; then + bias, the ReLU, + resid, each one rounding,
 * then the rounding to out_dtype.  So relu = 1 gives max(., 0) of the bits relu = 0 gives.  `groups` > 1: the four hypernetwork MLPs of the decoder in
 * one launch (row r = problem * 4 + mask token).  K % 8 == 0, K <= 2048 (VDR_ERR_UNSUPPORTED); anything else VDR_ERR_INVALID. */
int vdr_op_token_linear(const void* x, int64_t ldx, const void* x_add, int64_t ldxa, const void* W, const float* bias,
                        const void* resid, int64_t ldr, void* y, int out_dtype, int64_t ldy, int M, int N, int K, int groups,
                        int relu, void* stream);

/* The fused tail of the mask decoder's upscaling: GELU -> ConvTranspose2d(64, 32, kernel 2, stride 2) -> GELU -> the product
 * with the problem's hypernetwork outputs -> low-resolution logits.  The 32-channel 4g x 4g map is never written.
 *   x      device bf16 [problems*g*g*4, 64]: row (p*g*g + cy*g + cx)*4 + dy1*2 + dx1 is pixel (2cy+dy1, 2cx+dx1) of the 2g x 2g
 *          map after LayerNorm2d (the first transposed convolution as a linear on the weight reshaped to [4*64, C], then
 *          vdr_op_layernorm at D = 64).  gelu_in = 1: a = bf16(gelu(float(x))) is applied on load (the library's device
 *          polynomial, csrc/vdr_dev.h gelu_erf; pinned by the GELU tests of the GEMM epilogue); 0: a = x
 *   W      device bf16 [4*32, 64]: row (dy2*2+dx2)*32 + c = ConvTranspose2d.weight[:, c, dy2, dx2];  bias fp32 [32]
 *   hyper  device fp32 [problems, 4, 32]
 *   out    device fp32 [problems, 4, 4g, 4g]:
 *          u_c = gelu(sum_k a_k W[s2*32+c, k] + bias[c])   (fp32 MFMA accumulation over k, one addition, the polynomial)
 *          out[p, m, 2(2cy+dy1)+dy2, 2(2cx+dx1)+dx2] = (sum over c in C0 of hyper[p,m,c] u_c) + (sum over c in C1), each an fma
 *          chain from 0 in ascending c; C0 = channels with (c & 4) == 0, C1 the others (the two half-waves of the MFMA tile).
 * g in [1, 64] (VDR_ERR_UNSUPPORTED); null or misaligned (16 bytes) pointers, problems <= 0: VDR_ERR_INVALID. */
int vdr_op_mask_upscale(const void* x, const void* W, const float* bias, const float* hyper, float* out, int problems, int g,
                        int gelu_in, void* stream);

/* ---- the mask decoder object: SAM's box-prompt encoder and mask decoder as ONE call on the neck output of the image encoder.
 * A handle of its own: the vdr_weight_name enumeration, the workspace size and the launches of a vdr_handle do not change.
 * The arithmetic is the composition of the ops above with vdr_op_linear and vdr_op_layernorm (csrc/vdr_api.hip vdr_mask_decode;
 * DESIGN 4.3c); a "problem" is one (image, box) pair, P = batch * boxes_per_image.
 *   config: what segment_anything's MaskDecoder / TwoWayTransformer are built with.  The kernels cover channels 256, heads 8,
 *   depth 2, attention_downsample_rate 2, mask_tokens 4, upscale channels 64 / 32, iou_head_depth 3, mlp_dim any multiple of 64 up
 *   to 2048, grid 1 .. 64 (anything else: VDR_ERR_UNSUPPORTED).  img: the side of the input image the boxes are given in.
 *   ln_eps: the four LayerNorms of each two-way block (segment_anything 1e-5; transformers.SamModel applies 1e-6);
 *   final_ln_eps: norm_final_attn (1e-5 in both); ln2d_eps: the upscaling's LayerNorm2d (1e-6 in both).
 *   weights: segment_anything's names (vdr_mask_decoder_weight_name enumerates them, vdr_mask_decoder_num_weights counts), host
 *   fp32, any shape with the right element count; VDR_ERR_UNKNOWN_NAME otherwise.  vdr_mask_decoder_finalize rounds the GEMM
 *   weights to bf16, stacks the projections, builds the positional-encoding tables in float64 (VDR_ERR_INCOMPLETE: a weight is
 *   missing) and frees the host copies.
 *   vdr_mask_decode: emb device fp32 [batch, 256, g, g] (channels_last = 0) or [batch, g, g, 256] (1: the encoder's own
 *   VDR_OUT_ENCODER layout); boxes device fp32 [batch, boxes_per_image, 4] (x0, y0, x1, y1) in pixels of the img x img input;
 *   logits device fp32 [P, 4, 4g, 4g] and iou device fp32 [P, 4], all four mask tokens (token 0: the single-mask output, 1 .. 3:
 *   the multi-mask ones).  50 launches + 2 of set-up on `stream`, whatever batch and boxes_per_image; no host synchronisation, no
 *   allocation, no atomics; a problem's bits depend neither on P nor on its position.  Every refusal comes before the device is
 *   touched; a workspace smaller than vdr_mask_decoder_workspace_bytes(P) is VDR_ERR_WORKSPACE before anything is written, and
 *   nothing past that size is. */
typedef struct {
  int32_t grid, img, channels, heads, depth, mlp_dim, attention_downsample_rate, mask_tokens, upscale_channels_1, upscale_channels_2,
      iou_head_depth;
  float ln_eps, final_ln_eps, ln2d_eps;
} vdr_mask_decoder_config;
typedef struct vdr_mask_decoder* vdr_mask_decoder_handle;
int vdr_mask_decoder_create(const vdr_mask_decoder_config* cfg, int device, vdr_mask_decoder_handle* out);
void vdr_mask_decoder_destroy(vdr_mask_decoder_handle d);
int vdr_mask_decoder_num_weights(vdr_mask_decoder_handle d);
const char* vdr_mask_decoder_weight_name(vdr_mask_decoder_handle d, int i);
int vdr_mask_decoder_set_weight(vdr_mask_decoder_handle d, const char* name, const float* host, const int64_t* shape, int ndim);
int vdr_mask_decoder_finalize(vdr_mask_decoder_handle d);
int vdr_mask_decoder_workspace_bytes(vdr_mask_decoder_handle d, int problems, size_t* out);
int vdr_mask_decode(vdr_mask_decoder_handle d, const float* emb, int channels_last, const float* boxes, int batch, int boxes_per_image,
                    void* workspace, size_t workspace_bytes, float* logits, float* iou, void* stream);

/* ---- point and mask prompts (csrc/mask_prompt.hip).  Everything here is additive: the entry points above keep
 * their behaviour, their bits and their launches.
 *
 * Optional prompt weights.  vdr_mask_decoder_set_weight also accepts, before finalize, the names the second enumeration
 * (vdr_mask_decoder_num_prompt_weights / vdr_mask_decoder_prompt_weight_name) lists:
 *   points  prompt_encoder.point_embeddings.{0,1}.weight [1, 256], prompt_encoder.not_a_point_embed.weight [1, 256]
 *   mask    prompt_encoder.mask_downscaling.0.{weight [4,1,2,2], bias [4]}, .1.{weight, bias} [4], .3.{weight [16,4,2,2], bias [16]},
 *           .4.{weight, bias} [16], .6.{weight [256,16,1,1], bias [256]}   (mask_in_chans = 16)
 * finalize succeeds without them; a group given in part is VDR_ERR_INCOMPLETE naming the missing tensor.
 * vdr_mask_decoder_prompt_support: VDR_PROMPT_POINTS | VDR_PROMPT_MASK of a finalized handle.  The mask-prompt weights stay fp32.
 *
 * vdr_mask_prompts: device pointers.  boxes [batch, nb, 4] or NULL; points [batch, nb, np, 2] (x, y) in input pixels or NULL, labels
 * int32 [batch, nb, np], np = points_per_problem; mask_input fp32 [P, 4g, 4g], or [batch, 4g, 4g] with mask_per_image = 1 (shared by
 * the image's nb problems: transformers' form), or NULL.  At least one of boxes / points (VDR_ERR_INVALID).
 * Tokens per problem, segment_anything's layout: [iou; 4 mask tokens; np points; one padding point if boxes is NULL; the 2 box
 * corners otherwise], T = 5 + np + (boxes ? 2 : 1) <= 16 (more: VDR_ERR_UNSUPPORTED).
 * A point row: the Fourier features of ((x + 0.5) / img, (y + 0.5) / img), float64, as the box corners get them; label 1 / 0:
 * float(pe + point_embeddings[label]); -1: not_a_point_embed alone; -10: a zero row (transformers' padding); any other value: float(pe)
 * (transformers' behaviour; labels are not validated on the device).  The padding point is a label -1 row.  One rounding to bf16.
 * Keys: with mask_input bf16(emb + dense) by vdr_op_mask_embed (eps = ln2d_eps), else bf16(emb + no_mask_embed) as vdr_mask_decode.
 * vdr_mask_decode_prompts: vdr_mask_decode's contract -- 52 launches whatever the prompts, no host synchronisation, no allocation, no
 * atomics, a problem's bits depend neither on P nor on its position; every refusal before the device is touched; a workspace
 * below vdr_mask_decoder_workspace_bytes_prompts(P, T) is VDR_ERR_WORKSPACE with nothing written (equal to
 * vdr_mask_decoder_workspace_bytes at T = 7).  Points (or no boxes: the padding point) / a mask on a handle without their weights:
 * VDR_ERR_UNSUPPORTED.  With boxes only it gives vdr_mask_decode's bits.  The prompts themselves (none given, T > 16) are checked
 * first of all.  The workspace begins with the tokens as set up, bf16 [P, T, 256] (they double as the query positional encoding and
 * are not written again): the tests read the point rows there. */
#define VDR_PROMPT_POINTS 1
#define VDR_PROMPT_MASK 2
typedef struct {
  const float* boxes;
  const float* points;
  const int32_t* labels;
  int32_t points_per_problem;
  const float* mask_input;
  int32_t mask_per_image;
} vdr_mask_prompts;
int vdr_mask_decoder_num_prompt_weights(vdr_mask_decoder_handle d);
const char* vdr_mask_decoder_prompt_weight_name(vdr_mask_decoder_handle d, int i);
int vdr_mask_decoder_prompt_support(vdr_mask_decoder_handle d);
int vdr_mask_decoder_workspace_bytes_prompts(vdr_mask_decoder_handle d, int problems, int tokens, size_t* out);
int vdr_mask_decode_prompts(vdr_mask_decoder_handle d, const float* emb, int channels_last, const vdr_mask_prompts* prompts, int batch,
                            int boxes_per_image, void* workspace, size_t workspace_bytes, float* logits, float* iou, void* stream);

/* The fused keys of a decode with a mask prompt: keys[p * n + cell, c] = bf16(emb[p / nb, c, cell] + dense[c]), dense never written.
 *   emb      device fp32 [B, 256, g, g] (channels_last = 0) or [B, g, g, 256] (1); problem p reads image p / problems_per_image
 *   mask     device fp32 [problems, 4g, 4g], or [B, 4g, 4g] with mask_per_image = 1 (problem p reads mask p / problems_per_image)
 *   weights  device fp32 [VDR_MASK_EMBED_WEIGHTS]: mask_downscaling's 0.weight [4,1,2,2], 0.bias, 1.weight, 1.bias [4], 3.weight
 *            [16,4,2,2], 3.bias, 4.weight, 4.bias [16], 6.weight [256,16], 6.bias [256], back to back
 *   keys     device bf16 [problems * g * g, 256]
 * Per cell (cy, cx), every operation fp32 and rounded once unless written fma (the file is compiled without contraction):
 *   x[by,bx][dy,dx] = mask[4cy + 2by + dy, 4cx + 2bx + dx]
 *   c1[ch]  = the fma chain from b1[ch] over k = 2dy + dx ascending: acc = fma(w1[ch][k], x[k], acc)          (per 2 x 2 block)
 *   LayerNorm over the 4 channels, two-pass: mean = (((c0 + c1) + c2) + c3) / 4; d = c - mean; var = (d0 d0 + d1 d1 + ..) / 4 in
 *           ascending order from 0; rstd = 1 / sqrt(var + eps) (IEEE); y = (d * rstd) * gamma + beta
 *   a1      = gelu(y): the library's device polynomial (csrc/vdr_dev.h gelu_erf)
 *   c2[co]  = the fma chain from b2[co] over k = 4 ci + 2 by + bx ascending: acc = fma(w2[co][k], a1[k], acc)
 *   LayerNorm over the 16 channels (sum ascending from 0, / 16, as above), a2 = gelu(.)
 *   dense[c] = the fma chain from b3[c] over k ascending: acc = fma(w3[c][k], a2[k], acc)
 *   keys    = bf16(dense[c] + emb): one addition, one rounding.  So w3 = 0 gives bf16(emb + b3) exactly.
 * Fixed order everywhere, no atomics: a problem's bits depend neither on `problems` nor on its position nor on the layout.
 * g in [1, 64] (VDR_ERR_UNSUPPORTED); null or misaligned (16 bytes) pointers, problems outside 1 .. 65535 or no multiple of
 * problems_per_image, eps <= 0: VDR_ERR_INVALID. */
#define VDR_MASK_EMBED_WEIGHTS 4684
int vdr_op_mask_embed(const float* emb, int channels_last, const float* mask, int mask_per_image, const float* weights, void* keys,
                      int problems, int problems_per_image, int g, float eps, void* stream);

/* The box of a logit map, for the next slice of a volume sweep: over the pixels with logit > threshold of plane p (H x W fp32 at
 * logits + p * plane_stride elements: token 0 of [P, 4, H, W] is read in place with plane_stride = 4 H W),
 *   x0 = minX * sx - margin, x1 = (maxX + 1) * sx + margin, sx = float(img) / float(W); y likewise with sy = float(img) / float(H);
 *   each one fp32 multiplication and one addition, then clamped to [0, img].  boxes [P, 4] fp32 (x0, y0, x1, y1), area [P] int32 the
 *   pixel count.  An empty mask returns prev[p] (fp32 [P, 4]) and area 0.  Integer reductions: exact, one workgroup per problem, one launch,
 *   no atomics.  Refused: null pointers, non-positive sizes, problems > 65535, a plane_stride below H W, margin < 0 or NaN
 *   (VDR_ERR_INVALID); H W > 2^31 - 1, img > 2^24 (VDR_ERR_UNSUPPORTED). */
int vdr_op_mask_box(const float* logits, int64_t plane_stride, const float* prev, float* boxes, int32_t* area, int problems, int H, int W,
                    int img, float margin, float threshold, void* stream);

/* ---- automatic mask generation: the statistics of candidate masks and box NMS (csrc/mask_stats.hip, csrc/nms.hip).
 *
 * vdr_op_mask_stats: for each of `planes` planes of fp32 logits H x W, the bilinear up-sampling to oh x ow is evaluated and
 * reduced to seven integers; the up-sampled plane is never written.  Plane p starts at
 *   logits + (p / planes_per_group) * group_stride + (p % planes_per_group) * plane_stride   (elements),
 * so with planes_per_group = 1 plane p starts at logits + p * group_stride (one token of [P, 4, H, W] read in place, as
 * vdr_op_mask_box takes it), with planes_per_group = planes at logits + p * plane_stride (group_stride is then not read), and
 * tokens 1 .. 3 of [P, 4, H, W] are planes_per_group = 3, plane_stride = H W, group_stride = 4 H W from logits + H W.
 * The arithmetic is torch's upsample_bilinear2d(align_corners=False) on the CPU, every operation fp32 and rounded once, no fma
 * (the file is compiled without contraction):
 *   sy  = float(H) / float(oh)                                   one IEEE division; sx = float(W) / float(ow)
 *   src = (float(oy) + 0.5f) * sy - 0.5f, then src < 0 ? 0 : src  an addition, a multiplication, a subtraction
 *   y0  = (int)src;  l1 = src - float(y0);  l0 = 1.0f - l1;  y1 = y0 + (y0 < H - 1);   the same in x
 *   v   = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d)   a = in[y0][x0], b = in[y0][x1], c = in[y1][x0], d = in[y1][x1];
 *                                                                 each product and each sum rounded
 *   t_hi = threshold + offset, t_lo = threshold - offset          each computed once
 *   counts int32 [planes, 3]: the pixels with v > t_hi, v > threshold, v > t_lo (a NaN counts nowhere)
 *   box    int32 [planes, 4]: min x, min y, max x, max y (inclusive) over v > threshold; an empty mask gives 0, 0, 0, 0
 *                             (transformers' _batched_mask_to_box)
 * Integer reductions only: exact and independent of order.  Two launches (a partial slot per band of at most 32 output rows, then a
 * finish of one wave per plane in fixed order), no atomics, one writer per output; a plane's outputs depend neither on `planes` nor
 * on its position.  workspace: the partial slots, vdr_mask_stats_workspace_bytes (0 for a shape the op refuses); fewer bytes:
 * VDR_ERR_WORKSPACE, nothing written.  Refused before the device is touched (VDR_ERR_INVALID): null pointers; workspace, counts or
 * box not 16-byte aligned, logits not 4-byte aligned; H, W outside 1 .. 256; oh, ow outside 1 .. 4096; planes outside 1 .. 65535 or
 * no multiple of planes_per_group; plane_stride < H W; a group_stride that lets a group's planes overlap the next group; offset < 0
 * or NaN. */
#define VDR_MASK_STATS_MAX_SIDE 256
#define VDR_MASK_STATS_MAX_OUT 4096
size_t vdr_mask_stats_workspace_bytes(int planes, int H, int W, int oh, int ow);
int vdr_op_mask_stats(const float* logits, int64_t plane_stride, int planes_per_group, int64_t group_stride, int planes, int H, int W, int oh,
                      int ow, float threshold, float offset, void* workspace, size_t workspace_bytes, int32_t* counts, int32_t* box,
                      void* stream);

/* vdr_op_nms: greedy non-maximum suppression of n boxes, torchvision's definition.
 *   boxes   device fp32 [n, 4] (x0, y0, x1, y1)
 *   order   device int32 [n]: a permutation of 0 .. n - 1 listing the boxes best first (a stable descending sort of the scores).  An
 *           entry outside 0 .. n - 1 is never used as an address; the outputs are then unspecified
 *   keep    device uint8 [n]: keep[i] = 1 if box i is kept, else 0
 *   kept    device int32 [n]: the kept box indices in `order`'s sequence, then -1 up to n
 *   count   device int32 [1]: the number of kept boxes
 * Every operation fp32 and rounded once (no contraction):
 *   area  = (x1 - x0) * (y1 - y0)
 *   w     = min(x1_i, x1_j) - max(x0_i, x0_j), w < 0 ? 0 : w;  h likewise;  inter = w * h
 *   iou   = inter / ((area_i + area_j) - inter)                   IEEE division
 * Walking `order`, a box is kept unless an EARLIER KEPT box has iou > iou_threshold with it: the comparison is strict, and the NaN of
 * two zero-area boxes does not suppress.  Two launches: the n x ceil(n / 64) matrix of 64-bit suppression words (on and above the
 * diagonal) into the workspace, then ONE wave that walks it 64 positions at a time (the rows of a block are loaded together and the rows
 * that are not kept masked out: measured faster than loading kept rows one after the other).  No atomics, bitwise reproducible.
 * workspace: vdr_nms_workspace_bytes(n) = 8 n ceil(n / 64) bytes (0 for an n the op refuses); fewer: VDR_ERR_WORKSPACE, nothing
 * written.  Refused before the device is touched (VDR_ERR_INVALID): null pointers; boxes or workspace not 16-byte aligned, order,
 * kept or count not 4-byte aligned; n outside 1 .. 4096; a NaN iou_threshold. */
#define VDR_NMS_MAX_BOXES 4096
size_t vdr_nms_workspace_bytes(int n);
int vdr_op_nms(const float* boxes, const int32_t* order, int n, float iou_threshold, void* workspace, size_t workspace_bytes, uint8_t* keep,
               int32_t* kept, int32_t* count, void* stream);

/* ---- connected components of mask planes (csrc/components.hip, csrc/components_map.h).
 *
 * A plane is H x W uint8, nonzero = set, H and W in 1 .. 4096, pixel index i = y * W + x.  connectivity is 4 (edge neighbours) or
 * 8 (edge and corner neighbours).  value selects the pixels whose components are taken: 1 the set pixels, 0 the clear pixels
 * (the complement: holes and background).  The ROOT of a selected pixel is the lowest pixel index of its component; a pixel that
 * is not selected has root -1.  The AREA of a component is its pixel count.  Both are functions of the partition alone: every
 * correct algorithm, and every order in which workgroups run, gives the same integers.  Labels 1, 2, .. in the order of the
 * components' first pixels (scipy.ndimage.label's numbering) are the rank of the root among the roots (vdr.components.relabel).
 *
 * vdr_op_mask_binarize: planes of fp32 logits H x W, addressed as vdr_op_mask_stats addresses them (plane_stride,
 *   planes_per_group, group_stride), -> out uint8 [planes, oh, ow]: 1 where the bilinear align_corners=False up-sampling is
 *   > threshold, else 0 (a NaN gives 0).  The arithmetic is vdr_op_mask_stats', operation for operation (the same ms_axis, the same
 *   blend order, no contraction): the set pixels are exactly the ones mask_stats counts as v > threshold and boxes.  One launch.
 *   It accepts the shapes vdr_mask_stats_workspace_bytes accepts; the workspace is never read or written -- pointer and size are only
 *   checked, so that the call has the shape of the other ops (vdr_mask_binarize_workspace_bytes
 *   is 16 for an accepted shape, 0 for a refused one; fewer bytes: VDR_ERR_WORKSPACE).  Refused (VDR_ERR_INVALID): null pointers,
 *   logits not 4-byte aligned, H, W outside 1 .. 256, oh, ow outside 1 .. 4096, planes outside 1 .. 65535 or no multiple of
 *   planes_per_group, plane_stride < H W, overlapping groups, a NaN threshold.
 *
 * vdr_op_connected_components: mask uint8 [planes, H, W] ->
 *   root   int32 [planes, H, W]   the root of each pixel (-1: not selected)
 *   area   int32 [planes, H, W]   the component's area at its root pixel, 0 everywhere else
 *   count  int32 [planes]         the number of components
 *   Three launches: 64 x 64 tiles labelled in LDS by union-find; unions across the seams between tiles (find + integer atomicMin
 *   on the label plane); every pixel follows its chain to the root, tile areas are added to their root's (integer atomicAdd).
 *   workspace: vdr_connected_components_workspace_bytes = 4 bytes per pixel (the label plane).
 *
 * vdr_op_mask_clean: mask uint8 [planes, H, W], min_area >= 0, connectivity, mode = a set of VDR_CLEAN_* bits ->
 *   out      uint8 [planes, H, W]  0 / 1; it may not overlap mask (refused)
 *   changed  int32 [planes]        bit 0: the hole step changed the plane; bit 1: the island / largest step did
 *   stats    int32 [planes, 5]     the area of out, then its inclusive box x0, y0, x1, y1; 0, 0, 0, 0 for an empty plane
 *                                  (vdr_op_mask_stats' box convention)
 *   The steps run in this order, each on the result of the one before:
 *     VDR_CLEAN_HOLES    every component of the CLEAR pixels with area < min_area becomes set (segment_anything's rule: a
 *                        component that touches the border is not spared)
 *     VDR_CLEAN_ISLANDS  every component of the SET pixels with area < min_area is cleared; if all of them are below it the
 *                        largest stays, ties going to the lowest root
 *     VDR_CLEAN_LARGEST  only the largest component of the set pixels stays, ties going to the lowest root (min_area is not read)
 *   ISLANDS together with LARGEST is refused.  mode 0 copies (nonzero -> 1) and gives the statistics.  An empty plane, or one
 *   with nothing to remove, comes back unchanged with changed 0.  Launches, fixed for a mode: 4 for HOLES, 5 for ISLANDS or
 *   LARGEST (else 1 copy), 1 finish.  workspace: vdr_mask_clean_workspace_bytes = 8 bytes per pixel (label and area planes) +
 *   16 bytes per plane (rounded up to 8) + 64 bytes per 4096 pixels of a plane (partial slots of changed / stats).  The slots
 *   scale with the pixels: 8 + 1 / 64 bytes a pixel in all, not 8 plus a per-plane part only -- the price of one writer per
 *   statistic instead of per-plane atomics.
 *
 * The library's usual contract: plain device pointers, the caller's stream, no host synchronisation, no allocation; a plane's
 * outputs depend neither on `planes` nor on its position.  The integer atomics (minimum, sum) are order-independent: the outputs
 * are bitwise reproducible.  A workspace below the *_workspace_bytes (0 for a shape the op refuses): VDR_ERR_WORKSPACE, nothing
 * written.  Refused before the device is touched (VDR_ERR_INVALID): null pointers; H, W outside 1 .. 4096; planes outside
 * 1 .. 65535; a connectivity other than 4 and 8; a value other than 0 and 1; min_area < 0; unknown mode bits; ISLANDS | LARGEST;
 * out overlapping mask; a workspace not 16-byte aligned, int32 outputs not 4-byte aligned. */
#define VDR_COMPONENTS_MAX_SIDE 4096
#define VDR_CLEAN_HOLES 1
#define VDR_CLEAN_ISLANDS 2
#define VDR_CLEAN_LARGEST 4
size_t vdr_mask_binarize_workspace_bytes(int planes, int H, int W, int oh, int ow);
int vdr_op_mask_binarize(const float* logits, int64_t plane_stride, int planes_per_group, int64_t group_stride, int planes, int H, int W, int oh,
                         int ow, float threshold, void* workspace, size_t workspace_bytes, uint8_t* out, void* stream);
size_t vdr_connected_components_workspace_bytes(int planes, int H, int W);
int vdr_op_connected_components(const uint8_t* mask, int planes, int H, int W, int connectivity, int value, void* workspace, size_t workspace_bytes,
                                int32_t* root, int32_t* area, int32_t* count, void* stream);
size_t vdr_mask_clean_workspace_bytes(int planes, int H, int W);
int vdr_op_mask_clean(const uint8_t* mask, int planes, int H, int W, int min_area, int connectivity, int mode, void* workspace,
                      size_t workspace_bytes, uint8_t* out, int32_t* changed, int32_t* stats, void* stream);

/* ---- exact Euclidean distance transform of mask planes (csrc/edt.hip, csrc/edt_map.h).
 *
 * A plane is H x W uint8, nonzero = set, H and W in 1 .. 4096 (a zero-area plane is refused), planes in 1 .. 65535, pixel index
 * i = y * W + x.  value selects the pixels that are measured: 1 the set pixels, 0 the clear ones (vdr_op_connected_components'
 * convention).  Everything is an integer and a function of the mask alone: the outputs are bit for bit
 * rint(scipy.ndimage.distance_transform_edt(selected) ^ 2) and its indices under the tie rule below.
 *
 * vdr_op_distance_transform: mask uint8 [planes, H, W], value, outside, r2 -> four outputs, EACH OPTIONAL (null: not computed,
 * not touched), at least one of them given:
 *   d2       int32 [planes, H, W]  for a selected pixel (y, x): min (y - y')^2 + (x - x')^2 over the pixels (y', x') that are NOT
 *                                  selected; 0 on a pixel that is not selected.  outside = 1: everything beyond the plane counts as
 *                                  not selected, so the minimum also runs over (y + 1)^2, (H - y)^2, (x + 1)^2 and (W - x)^2.
 *                                  A selected pixel with no candidate at all (every pixel of the plane selected, outside = 0) gets
 *                                  VDR_EDT_NONE = 2^31 - 1.  The largest real value is 2 * 4095^2.
 *   nearest  int32 [planes, H, W]  the LOWEST pixel index among the non-selected pixels that attain the minimum; -1 on a pixel that
 *                                  is not selected and where there is none.  Refused together with outside = 1 (the nearest point
 *                                  may lie beyond the plane).  The tie rule is the separable form's own: within a row the nearest
 *                                  non-selected pixel with the lower x, across rows the lowest y'.
 *   peak     int32 [planes, 2]     the maximum of d2 over the plane and the lowest pixel index that attains it; (0, -1) for a plane
 *                                  with nothing selected.  VDR_EDT_NONE counts as a value: a full plane gives (VDR_EDT_NONE, 0).
 *   within   uint8 [planes, H, W]  1 where d2 <= r2, else 0, for r2 >= 0 (r2 is read only when within is given; a pixel that is not
 *                                  selected has d2 = 0 and is always 1).  Given WITHOUT d2 it takes d2's place: the int32 plane is
 *                                  never written -- Euclidean dilation and erosion by a radius r are this output at r2 = floor(r^2).
 *   The signature chosen for the thresholded plane is "a nullable d2 plus this output", not a mode flag: both may be asked at once.
 *
 * Two launches, three with peak: a row pass (per pixel the signed offset to the nearest non-selected pixel of its own row, 16 bits,
 * -32768 for "none in this row", which is tested for and never squared); a column pass that searches outwards from each pixel's own
 * row and stops when k^2 reaches the best so far (integer only; at most max(y, H - 1 - y) steps); with peak, one partial slot per
 * tile of the column pass and one wave per plane that reduces them.  No atomics.  No intermediate exceeds 2 * 4099^2 < 2^26.
 * workspace: vdr_distance_transform_workspace_bytes = 2 bytes a pixel (the row offsets; the total rounded up to 16) + 8 bytes per
 * 64 x 16 tile of a plane (the peak's slots): 2 + 1 / 128 bytes a pixel on large planes, not 2 plus a per-plane part only -- the
 * price of one writer per slot instead of a per-plane atomic maximum, as in vdr_op_mask_clean.
 *
 * The library's usual contract: plain device pointers, the caller's stream, no host synchronisation, no allocation; a plane's
 * outputs depend neither on `planes` nor on its position.  A workspace below the size (0 for a shape the op refuses):
 * VDR_ERR_WORKSPACE, nothing written.  Refused before the device is touched (VDR_ERR_INVALID): a null mask or workspace; all four
 * outputs null; H, W outside 1 .. 4096; planes outside 1 .. 65535; a value or an outside other than 0 and 1; nearest with
 * outside = 1; within with r2 < 0; a workspace not 16-byte aligned, int32 outputs not 4-byte aligned. */
#define VDR_EDT_MAX_SIDE 4096
#define VDR_EDT_NONE 2147483647
size_t vdr_distance_transform_workspace_bytes(int planes, int H, int W);
int vdr_op_distance_transform(const uint8_t* mask, int planes, int H, int W, int value, int outside, int r2, void* workspace, size_t workspace_bytes,
                              int32_t* d2, int32_t* nearest, int32_t* peak, uint8_t* within, void* stream);

/* ---- exact 3-D Euclidean distance transform of mask volumes with voxel spacing (csrc/edt3d.hip, csrc/edt3d_map.h).
 *
 * A volume is Z x H x W uint8, nonzero = set, every side in 1 .. 4096, voxel index i = (z H + y) W + x; there are `volumes` of
 * them, back to back.  value selects the voxels that are measured: 1 the set voxels, 0 the clear ones.  spacing is three INTEGERS
 * (qz, qy, qx), each in 1 .. 65535, in a unit the caller chooses (vdr.morphology.quantize_spacing: millimetres / 2^-10, say); the
 * squared distance between two voxels (dz, dy, dx) apart is (qz dz)^2 + (qy dy)^2 + (qx dx)^2.  Everything is an integer and a
 * function of the mask and the spacing alone.  The bound (qz Z)^2 + (qy H)^2 + (qx W)^2 <= 2^53 makes every value exact both in
 * int64 and in float64, so the outputs are bit for bit rint(scipy.ndimage.distance_transform_edt(selected, sampling=(qz, qy, qx)) ^ 2),
 * and scipy's float64 result is exactly sqrt(d2).
 *
 * vdr_op_distance_transform_3d: vol uint8 [volumes, Z, H, W], spacing, value, outside, r2 -> three outputs, EACH OPTIONAL (null: not
 * computed, not touched), at least one of them given:
 *   d2      int64 [volumes, Z, H, W]  for a selected voxel: min (qz dz)^2 + (qy dy)^2 + (qx dx)^2 over the voxels that are NOT selected;
 *                                     0 on a voxel that is not selected; VDR_EDT3_NONE = 2^63 - 1 on a selected voxel with no
 *                                     candidate at all.  The largest real value is at most 2^53.
 *   peak    int64 [volumes, 2]        the largest d2 of a volume and the lowest voxel index that attains it; (0, -1) for a volume with
 *                                     nothing selected.  VDR_EDT3_NONE counts as a value: a full volume with outside = 0 gives
 *                                     (VDR_EDT3_NONE, 0).
 *   within  uint8 [volumes, Z, H, W]  1 where d2 <= r2, else 0, for r2 >= 0 (read only when within is given; a voxel that is not
 *                                     selected has d2 = 0 and is always 1).  Given WITHOUT d2 it takes d2's place and no int64 volume
 *                                     is written: Euclidean dilation and erosion by the ellipsoid of a radius r are this output at
 *                                     r2 = floor(r^2 / unit^2).
 *   outside 0 .. 7, one bit an axis: bit 2 = z, bit 1 = y, bit 0 = x.  On a set axis everything beyond the volume's two faces counts
 *           as not selected: the minimum also runs over (q (c + 1))^2 and (q (side - c))^2 of that axis.  Scan volumes are routinely
 *           cropped along z only, which is why this is per axis.
 *   Out of scope: `nearest` in 3-D (it needs a tie rule of its own); spacing that differs per volume of one call.
 *
 * Three launches, four with peak: the x pass is vdr_op_distance_transform's row pass over the volumes * Z planes (the signed 16-bit
 * row offset); the y pass searches outwards along y with the weights (qy, qx), stops when (qy k)^2 reaches the best so far, and leaves
 * per voxel the in-plane VECTOR (oy, ox) as two int16 (4 bytes, not the 8 of the value); the z pass searches outwards over the slices
 * z +- k, recomputing the in-plane value from the vector, and stops when (qz k)^2 reaches the best so far (at most max(z, Z - 1 - z)
 * steps); with peak, one partial slot per tile of the z pass and one wave per volume that reduces them.  No atomics.  A weighted
 * step q k is below 2^32 and its square is one 32 x 32 -> 64 multiply; sums stay below 2^60; compares are int64.
 * When within is asked for ALONE (no d2, no peak) the searches also end early: the y search when (qy k)^2 > r2, the z search when
 * best <= r2 or (qz k)^2 > r2 -- nothing further out can change d2 <= r2.  This changes no output bit and bounds a dilation or an
 * erosion by a small radius to O(r) steps.  (The y search may NOT stop at best <= r2: a row further out can still be nearer in the
 * plane, and a voxel some slices away may need exactly that difference.)
 * workspace: vdr_distance_transform_3d_workspace_bytes = 2 bytes a voxel (row offsets) + 4 bytes a voxel (vectors), each section
 * rounded up to 16, + 16 bytes per 64 x 16 tile of a slice (the peak's slots); 0 for a shape the op refuses.
 *
 * The library's usual contract: plain device pointers, the caller's stream, no host synchronisation, no allocation; a volume's
 * outputs depend neither on `volumes` nor on its position.  A workspace below the size: VDR_ERR_WORKSPACE, nothing written.  Refused
 * before the device is touched (VDR_ERR_INVALID): a null vol or workspace; all three outputs null; volumes < 1; Z, H, W outside
 * 1 .. 4096; volumes * Z above 65535; Z * H * W above 2^30; a spacing outside 1 .. 65535; (qz Z)^2 + (qy H)^2 + (qx W)^2 > 2^53; a
 * value other than 0 and 1; outside outside 0 .. 7; within with r2 < 0; a workspace not 16-byte aligned, int64 outputs not 8-byte
 * aligned. */
#define VDR_EDT3_NONE 9223372036854775807ll
#define VDR_EDT3_MAX_SPACING 65535
size_t vdr_distance_transform_3d_workspace_bytes(int volumes, int Z, int H, int W);
int vdr_op_distance_transform_3d(const uint8_t* vol, int volumes, int Z, int H, int W, int qz, int qy, int qx, int value, int outside, int64_t r2,
                                 void* workspace, size_t workspace_bytes, int64_t* d2, int64_t* peak, uint8_t* within, void* stream);

/* SAM / MedSAM Attention.forward with use_rel_pos (third-party segment_anything ImageEncoderViT, called at
 * tfds_dense_descriptor.py:123): per (window, head) softmax(q k^T dh^-0.5 + q.Rh[qh-kh] + q.Rw[qw-kw]) v.
 *   qkv   [batch*S*S, 3*H*64] bf16, `batch` windows (or whole grids) of S x S tokens, row-major (h, w)
 *   rel_pos_h / rel_pos_w  fp32 [2S-1, 64] (the block's parameters)
 *   rel   device scratch, fp32 [batch*S*S*H*Np + Np*32], Np = 2*roundup(2S-1, 32): the products of q with
 *         every relative-offset row of both tables (one MFMA GEMM) and, behind them, the packed bf16 tables
 *   out   [batch*S*S, H*64] bf16.   Any S in 1..64: {4, 7, 10, 14} one pass and 64 online softmax with compile-time
 *         key coordinates, every other S the run-time-grid kernel (online softmax over 128-key chunks, ragged last
 *         chunk).  S > 64: VDR_ERR_UNSUPPORTED (the packed operand holds 127 + 127 rows). */
int vdr_op_attention_relpos(const void* qkv, const float* rel_pos_h, const float* rel_pos_w, float* rel, void* out,
                            int batch, int S, int heads, void* stream);

/* ---- the window path of a SAM / MedSAM block and the neck's 3 x 3 convolution, step by step -----------------------------
 * segment_anything Block.forward: norm1, window_partition, attention, window_unpartition, the residual add; Neck: the
 * second Conv2d (3 x 3, padding 1).  Each entry point is the argument builder and the launcher vdr_forward itself runs
 * for that step (csrc/vdr_api.hip: sam_ln_args, sam_ln_mx, sam_proj_args, launch_im2col3), on caller buffers.
 * Geometry: `batch` images of g x g tokens, row b*g*g + y*g + x ("token order"); ws x ws windows, nw = ceil(g / ws) a side,
 * the last window of a row / column padded when ws does not divide g (g < ws: one partly filled window).  "Windowed
 * order" is window_partition's: row ((b*nw + y/ws)*nw + x/ws)*ws*ws + (y%ws)*ws + x%ws, wrows = batch*nw*nw*ws*ws rows in
 * all; rows whose (y, x) falls outside the grid are padding rows.
 * Refused before the device is touched: null pointers ("null argument"), batch < 1, g < 1, ws < 1 ("bad shape"), 2^31 or
 * more windowed rows, a pointer that is not 16-byte aligned (VDR_ERR_INVALID); the width constraints named below
 * (VDR_ERR_UNSUPPORTED). */

/* norm1 + window_partition: x bf16 [batch*g*g, D], token order -> y bf16 [wrows, D], windowed order; gamma / beta fp32 [D].
 * Row arithmetic and bits of vdr_op_layernorm.  Padding rows of y are NOT written: the caller zeroes them (vdr_forward: one
 * memset per forward).  D % 4 == 0, D <= 2048. */
int vdr_op_layernorm_window(const void* x, void* y, const float* gamma, const float* beta, int batch, int g, int ws, int D,
                            float eps, void* stream);
/* The same with MX-fp8 output (vdr_op_layernorm_mx's arithmetic): payload q [wrows, D] bytes, scales the array of an MX
 * tensor of wrows rows (vdr_mx_scale_bytes(wrows, D); row r of the WINDOWED order owns the bytes the layout above gives
 * row r).  Payload and scale bytes of padding rows, and the scale bytes of rows wrows .. rows_pad - 1, are not written.
 * D % 32 == 0, D <= 2048. */
int vdr_op_layernorm_mx_window(const void* x, const float* gamma, const float* beta, float eps, int batch, int g, int ws, int D,
                               void* q, void* scales, void* stream);
/* attn.proj + window_unpartition + the residual add: y[t] = resid[t] + x[m] . W^T + bias for every windowed row m that is
 * no padding row, t its token-order row.
 *   x [wrows, K] bf16, windowed order (padding rows are multiplied but dropped: any bits, NaN included);  W [N, K] bf16
 *   (PyTorch layout, as vdr_op_linear);  bias fp32 [N] or NULL;  resid, y bf16 [batch*g*g, N], token order; y may be resid
 *   variant: 0 = the tile variant vdr_forward picks for this out-projection, or 22..29
 *   part non-NULL (N % 64 == 0, part_stride >= batch*g*g): the LayerNorm partials of y's rows as vdr_op_linear_ln_stats
 *   writes them, part [N/64][part_stride][2] fp32, indexed by the TOKEN-order row; rows >= batch*g*g are not written.
 * K % 64 == 0, N % 8 == 0.  A valid row's bits are those of vdr_op_linear (VDR_EPI_BIAS_RESID) on the same variant. */
int vdr_op_linear_window(const void* x, const void* W, const float* bias, const void* resid, void* y, int batch, int g, int ws,
                         int N, int K, int variant, float* part, int64_t part_stride, void* stream);
/* The neck's 3 x 3 / padding 1 im2col: x bf16 [batch*g*g, C] (NHWC tokens) -> col bf16 [batch*g*g, 9*C], tap-major:
 * col[r][(ky*3 + kx)*C + c] = x[(b, y + ky - 1, x + kx - 1)][c], zero outside the image's own grid -- the operand layout
 * "neck.2.weight" is packed for ([C_out][(ky*3 + kx)*C_in + c]).  Pure data movement.  C % 8 == 0. */
int vdr_op_im2col3(const void* x, void* col, int batch, int g, int C, void* stream);

/* DINOv2 / transformers interpolate_pos_encoding: the patch rows of a learned position table resampled from a
 * gh0 x gw0 grid to gh x gw (bicubic, A = -0.75, align_corners = False, size = (gh, gw), no antialias, border
 * indices clamped).  pos, out: device fp32, [gh0*gw0, D] and [gh*gw, D], row-major over (y, x).  No CLS row.
 * Source coordinate (o + 0.5) * (g0 / g) - 0.5, the cubic-convolution weights and the 16-tap sum are evaluated in
 * fp64 and rounded to fp32 once: the result is F.interpolate(table.double(), size=(gh, gw), mode="bicubic",
 * align_corners=False) rounded once (torch's fp32 path rounds the source coordinate to fp32 and differs by a few ulp).
 * At most 2^20 grid cells either side. */
int vdr_op_interpolate_pos(const float* pos, int gh0, int gw0, int D, float* out, int gh, int gw, void* stream);

/* segment_anything get_rel_pos (also transformers' SamVisionAttention): a relative-position table resampled along its
 * row axis, per channel -- F.interpolate(table[L0, D] as [1, D, L0], size = L, mode = "linear", align_corners = False).
 * table, out: device fp32, [L0, D] and [L, D].  src = max((i + 0.5) * L0 / L - 0.5, 0), i0 = trunc(src), the upper
 * neighbour clamped at the last row, weights (1 - t, t) with t = src - i0; evaluated in fp64 and rounded to fp32 once.
 * A SAM table for grid side g has L = 2 g - 1 rows.  At most 2^30 elements either side. */
int vdr_op_interpolate_rel_pos(const float* table, int L0, int D, float* out, int L, void* stream);

/* DINOv3's axial 2-D rotary position embedding (transformers DINOv3ViTRopePositionEmbedding): the cos / sin tables of a
 * gh x gw patch grid, device fp32 [gh*gw, head_dim/2] each -- the unique half; the upper half of a head repeats it.
 * inv_freq[i] = theta^(-4 i / head_dim), i < head_dim/4.  Patch (y, x): cy = 2 (y + 0.5) / gh - 1, cx = 2 (x + 0.5) / gw - 1;
 * angle[j] = 2 pi cy inv_freq[j] for j < head_dim/4, 2 pi cx inv_freq[j - head_dim/4] above.  Angle, cos and sin are evaluated
 * in fp64 and rounded to fp32 once (transformers' fp32 table differs by <= 7e-7).  Load-time class.  head_dim in
 * {32, 64, 128} (else VDR_ERR_UNSUPPORTED); theta finite and > 1, at most 2^20 grid cells (VDR_ERR_INVALID). */
int vdr_op_rope2d_table(int gh, int gw, int head_dim, float theta, float* cos_out, float* sin_out, void* stream);

/* apply_rotary_pos_emb on the patch rows of a packed qkv activation, in place: qkv [batch*seq, 3*H*dh] bf16, columns
 * [q | k | v] each [H, dh].  Only rows b*seq + prefix + j (j < seq - prefix) are touched, with table row j, and in them only
 * the q and k columns; prefix rows and v are neither read nor written.  Per head and j2 < dh/2, with lo = t[j2],
 * hi = t[j2 + dh/2] (bf16, widened exactly), c = cos[j][j2], s = sin[j][j2], every operation one fp32 rounding, in this
 * order (no fused multiply-add):
 *   p1 = lo * c,  p2 = hi * s,  lo' = p1 - p2;    p3 = hi * c,  p4 = lo * s,  hi' = p3 + p4
 * lo' and hi' are rounded to bf16 once (nearest even) and stored over lo and hi (the rotate_half convention).  One lane:
 * 8 lo dims and their 8 partners, for q and for k (16-byte accesses); no LDS, no atomics: a row's result does not depend
 * on batch.  cos / sin: device fp32 [seq - prefix, dh/2] (vdr_op_rope2d_table, or any caller table).  qkv, cos, sin 16-byte
 * aligned.  head_dim in {32, 64, 128} (else VDR_ERR_UNSUPPORTED). */
int vdr_op_rope2d(void* qkv, int batch, int seq, int prefix, int heads, int head_dim, const float* cos, const float* sin,
                  void* stream);

/* nn.Conv2d(in_chans, D, kernel=p, stride=p) + flatten(2).transpose(1,2) — DINOv2 PatchEmbed,
 * the op called at tfds_dense_descriptor.py:128.
 *   images NCHW [batch, C, img, img] in_dtype; W bf16 [D, Kp] (C*p*p columns zero-padded to
 *   Kp = roundup(C*p*p, 64)); bias fp32 [D]; pos fp32 [n(+1), D] or NULL;
 *   col: device scratch of batch*n*Kp bf16 (left untouched when the images are bf16, 16-byte aligned and p is 8, 16
 *   or 32: the GEMM then gathers its operand from the images, no im2col pass);
 *   y bf16: row (b*row_stride + row_offset + i) for patch i of image b, plus pos[row_offset+i]. */
int vdr_op_patch_embed(const void* images, int in_dtype, const void* W, const float* bias,
                       const float* pos, void* col, void* y, int batch, int C, int img, int p, int D,
                       int row_stride, int row_offset, void* stream);

/* The same for nn.Conv2d(in_chans, D, kernel=p, stride=stride), stride | p, over [batch, C, H, Wd] images, (H - p) and
 * (Wd - p) multiples of stride: n = ((H - p) / stride + 1) * ((Wd - p) / stride + 1) overlapping patches in (y, x) order.
 * stride < p: col (batch*n*Kp bf16) is always written -- col[b*n + i][c*p*p + ky*p + kx] = the pixel rounded once to bf16,
 * columns C*p*p .. Kp-1 zero -- by the overlapping im2col of csrc/patch_stride.hip (LDS form: p even, stride >= 2, Wd a
 * multiple of 8 (p % 8 == 0) or 2, images 16-byte aligned; else one thread per 16-byte chunk).  stride == p:
 * vdr_op_patch_embed's paths (rectangular sizes through im2col). */
int vdr_op_patch_embed_strided(const void* images, int in_dtype, const void* W, const float* bias, const float* pos, void* col,
                               void* y, int batch, int C, int H, int Wd, int p, int stride, int D, int row_stride, int row_offset,
                               void* stream);
/* Log-binning of a dense descriptor map (csrc/log_bin.hip).  F[b, y, x, c] on a gh x gw grid, C channels, hierarchy h:
 *   A_k = mean of F over the 3^k x 3^k window centred at (y, x) intersected with the grid (divided by the in-grid count);
 *   bins: k = 0 .. h-1, dy in (-3^k, 0, +3^k), dx likewise, (0, 0) skipped for k >= 1 -- 1 + 8h bins;
 *   out[b, y*gw + x, j*C + c] = A_k[b, clamp(y + dy, 0, gh-1), clamp(x + dx, 0, gw-1), c], bin-major, [batch, gh*gw, (1+8h)*C].
 * x points at the first patch row's first channel; consecutive patch rows are ld elements apart, images image_stride
 * elements apart (in_dtype VDR_BF16 | VDR_F32).  Window sums are fixed-order fp32 additions without atomics (a value's
 * bits do not depend on the batch position or the launch), the mean is one IEEE fp32 division sum / count, bf16 output is
 * one rounding of that, level-0 bins are exact copies.  work: fp32 scratch of (h-1)*batch*gh*gw*C elements (NULL allowed
 * when h == 1).  Refused before the device is touched: VDR_ERR_INVALID for C % 8 != 0, ld < C, null pointers,
 * non-positive sizes, pointers or rows (ld, image_stride) that are not 16-byte aligned; VDR_ERR_UNSUPPORTED for a
 * hierarchy outside 1..3. */
int vdr_op_log_bin(const void* x, int in_dtype, int64_t ld, int64_t image_stride, int batch, int gh, int gw, int C,
                   int hierarchy, float* work, void* out, int out_dtype, void* stream);

/* Cosine nearest neighbours between two descriptor maps (csrc/nn_cosine.hip): for each of `pairs` problems, every row of
 * X_p against every row of Y_p, without the tx x ty similarity matrix ever being written.
 *   X_p = [tx, d] bf16, rows ldx elements apart, starting at x + p * x_stride; Y_p = [ty, d] bf16 with ldy and y_stride
 *   likewise.  A stride of 0 is allowed (one map matched against many).
 * Definition:
 *   ss(v)     = sum_c v_c^2 in fp32 (products of bf16 values are exact in fp32; fixed summation order, no atomics);
 *   rn(v)     = 1.0f / fmaxf(sqrtf(ss(v)), 1e-8f), correctly rounded sqrtf and division;
 *   sim(i, j) = (dot(x_i, y_j) * rn(x_i)) * rn(y_j), in this association; dot is accumulated in fp32 by bf16 MFMAs;
 *   row_sim[p, i] = max_j sim(i, j), row_idx[p, i] the lowest j that attains it        ([pairs, tx] fp32 / int32);
 *   col_sim[p, j] = max_i sim(i, j), col_idx[p, j] the lowest i that attains it        ([pairs, ty] fp32 / int32).
 * Comparisons are > on the value, then < on the index.  Inputs are finite by contract; a zero row has sim = 0 against
 * everything.  Results are bitwise reproducible from run to run, and a pair's result does not depend on `pairs` or on its
 * position in the batch.
 * col_sim == NULL && col_idx == NULL skips the column side.  work: vdr_nn_cosine_work_bytes(pairs, tx, ty) bytes of device
 * scratch (row norms and the partial maxima), 16-byte aligned.
 * Refused before the device is touched: VDR_ERR_UNSUPPORTED for d % 32 != 0; VDR_ERR_INVALID for a null x, y, work, row_sim
 * or row_idx, exactly one of col_sim / col_idx null, non-positive pairs, tx, ty or d, ldx < d or ldy < d, negative
 * strides, pointers or strides (ldx, ldy, x_stride, y_stride) that are not 16-byte aligned, pairs * max(tx, ty) above
 * 2^31 - 1. */
size_t vdr_nn_cosine_work_bytes(int pairs, int tx, int ty);
int vdr_op_nn_cosine(const void* x, int64_t ldx, int64_t x_stride, int tx,
                     const void* y, int64_t ldy, int64_t y_stride, int ty,
                     int pairs, int d, void* work,
                     float* row_sim, int32_t* row_idx, float* col_sim, int32_t* col_idx, void* stream);

/* k nearest neighbours between two descriptor maps (csrc/knn.hip): for each of `pairs` problems, the k best candidates of
 * every query over ALL candidates, without the tq x tc score matrix ever being written.
 *   X_p = [tq, d] bf16 (the queries), rows ldx elements apart, starting at x + p * x_stride; Y_p = [tc, d] bf16 (the
 *   candidates) with ldy and y_stride likewise.  A stride of 0 is allowed (many query sets against one bank).  The operand
 *   rules are vdr_op_nn_cosine's.
 * Definition, one fp32 rounding per step, in this order:
 *   ss(v), rn(v), dot = vdr_op_nn_cosine's: ss(v) = sum_c v_c^2 in fp32 in its fixed order, rn(v) = 1.0f / fmaxf(sqrtf(ss(v)),
 *               1e-8f) with correctly rounded sqrtf and division, dot accumulated in fp32 by bf16 MFMAs in ascending k;
 *   metric VDR_KNN_COSINE: s(i, j) = (dot(x_i, y_j) * rn(x_i)) * rn(y_j): two multiplications, in this association -- the bits
 *               of vdr_op_nn_cosine's sim(i, j).  Better means greater s, then lower j;
 *   metric VDR_KNN_L2:     s(i, j) = fmaxf(fmaf(-2.0f, dot(x_i, y_j), ss(x_i) + ss(y_j)), 0.0f): one addition, one fused
 *               multiply-add, the clamp -- the SQUARED distance; the square root is the caller's.  Better means smaller s, then
 *               lower j.  The value returned is s itself, never -0;
 *   exclude_diag != 0: candidate j == i is not eligible for query i (the k-NN graph of one map against itself);
 *   val[p, i, m], idx[p, i, m] = s and j of the m-th best eligible candidate of query i, m = 0 .. k - 1   ([pairs, tq, k]
 *               fp32 / int32), best first.
 * The order is total on pairs with distinct indices, so a problem's bits depend on (tq, tc, d, k, metric, exclude_diag,
 * inputs) only -- not on `pairs`, on its position in the batch or on how the launch cuts the candidates into runs.  Inputs are
 * finite by contract.  No atomics; every output element has exactly one writer.  With k = 1 and the cosine metric val / idx
 * equal vdr_op_nn_cosine's row_sim / row_idx bit for bit.
 * work: vdr_knn_work_bytes(pairs, tq, tc, k) bytes of device scratch (the row norms and the partial lists), 16-byte aligned;
 * it is written before it is read.
 * Refused before the device is touched, in this order: VDR_ERR_INVALID for a null x, y, work, val or idx, non-positive
 * pairs, tq, tc or d; VDR_ERR_UNSUPPORTED for d % 32 != 0; VDR_ERR_INVALID for ldx < d or ldy < d, negative strides,
 * pointers or strides that are not 16-byte aligned, pairs * max(tq, tc) above 2^31 - 1; VDR_ERR_UNSUPPORTED for k outside
 * 1 .. VDR_KNN_MAX_K; VDR_ERR_INVALID for an unknown metric, for tc - (exclude_diag ? 1 : 0) < k (so no padding entry is ever
 * returned: exactly k neighbours, always), for pairs * tq * k above 2^31 - 1. */
#define VDR_KNN_MAX_K 16
enum vdr_knn_metric { VDR_KNN_COSINE = 0, VDR_KNN_L2 = 1 };
size_t vdr_knn_work_bytes(int pairs, int tq, int tc, int k);
int vdr_op_knn(const void* x, int64_t ldx, int64_t x_stride, int tq, const void* y, int64_t ldy, int64_t y_stride, int tc,
               int pairs, int d, int k, int metric, int exclude_diag, void* work, float* val, int32_t* idx, void* stream);

/* Windowed correlation of two descriptor maps that live on ONE gh x gw grid (csrc/local_corr.hip): for each of `pairs`
 * problems, every patch of X_p against the patches of Y_p at most `radius` grid steps away in y and in x -- the search for
 * adjacent slices or a follow-up scan, where a structure moves by a few patches.  t = gh * gw, row i = qy * gw + qx.
 *   X_p = [t, d] bf16 (the queries), rows ldx elements apart, starting at x + p * x_stride; Y_p = [t, d] bf16 (the
 *   candidates) with ldy and y_stride likewise.  A stride of 0 is allowed.  The operand rules are vdr_op_nn_cosine's.
 * Definition, with W = 2 * radius + 1; slot w = (dy + radius) * W + (dx + radius) holds the displacement (dy, dx), dy and dx
 * in [-radius, radius]; the candidate of slot w for query i = (qy, qx) is j = (qy + dy) * gw + (qx + dx):
 *   ss, rn, dot = vdr_op_nn_cosine's: ss(v) = sum_c v_c^2 in fp32, rn(v) = 1.0f / fmaxf(sqrtf(ss(v)), 1e-8f) with correctly
 *               rounded sqrtf and division, dot accumulated in fp32 by bf16 MFMAs in ascending k;
 *   sim(i, j)   = (dot(x_i, y_j) * rn(x_i)) * rn(y_j), in this association: the bits are vdr_op_nn_cosine's sim(i, j);
 *                 with transposed != 0 it is (dot(x_i, y_j) * rn(y_j)) * rn(x_i) instead, the candidate's norm first: the
 *                 bits of vdr_op_nn_cosine's sim(j, i) for the operands exchanged -- the two multiplications do not
 *                 commute in fp32, and the reverse direction of a match (queries Y, candidates X) must not depend on
 *                 which of the two searches, the global or the windowed, produced it;
 *   cost[p, i, w]  = sim(i, j) when (qy + dy, qx + dx) is inside the grid, -inf otherwise      ([pairs, t, W * W] fp32);
 *   best_sim[p, i] = the maximum of cost[p, i, :] over the in-grid slots                        ([pairs, t] fp32);
 *   best_idx[p, i] = the lowest j that attains it (slots ascend with j: also the lowest slot)   ([pairs, t] int32).
 * Comparisons are > on the value, then < on the index.  Inputs are finite by contract.  No atomics; every entry of cost
 * has exactly one writer; a problem's bits depend on (gh, gw, radius, d, inputs) only -- not on `pairs`, on its position in
 * the batch or on a launch heuristic.  A window that covers the grid (radius >= max(gh, gw) - 1) gives best_sim / best_idx
 * equal to vdr_op_nn_cosine's row_sim / row_idx bit for bit, and with transposed != 0 equal to the col_sim / col_idx of
 * vdr_op_nn_cosine(y, x).
 * cost == NULL: only the best pair is wanted.  best_sim == NULL && best_idx == NULL: only the cost volume.  At least one
 * output must be given.  work: vdr_local_correlation_work_bytes(pairs, gh, gw, radius) bytes of device scratch (the row
 * norms, and room for the cost rows the best pair is folded from when cost == NULL), 16-byte aligned; it is written before
 * it is read.
 * Refused before the device is touched, in this order: VDR_ERR_INVALID for a null x, y or work, non-positive pairs, gh,
 * gw or d; VDR_ERR_UNSUPPORTED for d % 32 != 0; VDR_ERR_INVALID for ldx < d or ldy < d, negative strides, pointers or
 * strides that are not 16-byte aligned, pairs * t above 2^31 - 1, gh * gw above 2^31 - 1; VDR_ERR_UNSUPPORTED for a radius
 * outside 1 .. VDR_LOCAL_CORR_MAX_RADIUS; VDR_ERR_INVALID for no output at all, exactly one of best_sim / best_idx null,
 * outputs that are not 16-byte aligned, pairs * t * W * W above 2^31 - 1. */
#define VDR_LOCAL_CORR_MAX_RADIUS 8
size_t vdr_local_correlation_work_bytes(int pairs, int gh, int gw, int radius);
int vdr_op_local_correlation(const void* x, int64_t ldx, int64_t x_stride, const void* y, int64_t ldy, int64_t y_stride,
                             int pairs, int gh, int gw, int d, int radius, int transposed, void* work,
                             float* cost, float* best_sim, int32_t* best_idx, void* stream);

/* Multi-source soft window vote (csrc/window_vote.hip): DINO's label propagation step for one target map against S source
 * maps -- the annotated slice and the last few propagated ones --, soft labels in and out.  For each of `problems` problems
 * on one gh x gw grid, t = gh * gw, W = 2 * radius + 1:
 *   cost [problems, sources, t, W * W] fp32: the S cost volumes of the target against its sources, as
 *     vdr_op_local_correlation writes them (slot w = (dy + radius) * W + (dx + radius)); one call of it with pairs = S, the
 *     target at x_stride = 0 and the sources y_stride apart writes a problem's block.
 *   src  [problems, sources, t, n_classes] fp32: the class scores of the source patches, finite and non-negative by
 *     contract; one-hot rows are hard labels.
 * Definition, for query i = (qy, qx) of problem p:
 *   candidates  the pairs (s, w) whose position (qy + dy, qx + dx) is inside the grid -- decided from (gh, gw, radius); the
 *               values of the other slots are never read.  Candidate (s, w) has the patch index j = (qy + dy) * gw + (qx + dx)
 *               and the value cost[p, s, i, w].
 *   order       greater value first, then lower s, then lower w: total.  The neighbours m = 0 .. k-1 are the first k
 *               candidates under it (exact fp32 comparisons; nothing is rounded).
 *   weights     VDR_VOTE_SOFTMAX: e_m = expf((v_m - v_0) * inv_t), inv_t = 1.0f / temperature rounded once, the subtraction
 *               and the multiplication one fp32 rounding each; expf is the device math library's, whose error is at most
 *               1 ulp (a relative error of at most 2^-23; results below 2^-126 may be flushed to 0), and expf(0) = 1
 *               exactly, so e_0 is 1.0f.  VDR_VOTE_UNIFORM: e_m = 1 (temperature is checked all the same).
 *   scores[p, i, c] = (sum_m e_m * src[p, s_m, j_m, c]) / (sum_m e_m): every product rounded before it is added, both sums
 *               in fp32 ascending in m starting from the first term, one IEEE division per class.  ([problems, t, n_classes])
 *   labels[p, i] = the lowest c that attains the largest scores[p, i, c]                              ([problems, t] int32)
 *   idx[p, i, m] = s_m * t + j_m, a row of the problem's [sources * t, n_classes] src; val[p, i, m] = v_m  ([problems, t, k])
 * labels may be NULL; idx and val may be NULL, but only together.  No atomics; every entry has exactly one writer; a
 * problem's bits depend on (gh, gw, radius, sources, k, n_classes, weights, temperature, inputs) only -- not on `problems`,
 * on its position in the batch or on a launch heuristic.  No scratch memory is needed.
 * Refused before the device is touched, in this order: VDR_ERR_INVALID for a null cost, src or scores, non-positive
 * problems, sources, gh, gw or n_classes, pointers that are not 16-byte aligned, problems * sources * gh * gw above
 * 2^31 - 1; VDR_ERR_UNSUPPORTED for sources above VDR_WINDOW_VOTE_MAX_SOURCES, a radius outside 1 ..
 * VDR_LOCAL_CORR_MAX_RADIUS, k outside 1 .. VDR_WINDOW_VOTE_MAX_K, n_classes above VDR_WINDOW_VOTE_MAX_CLASSES;
 * VDR_ERR_INVALID for k above sources * min(gh, radius + 1) * min(gw, radius + 1) (the candidates of a corner patch: a slot
 * outside the grid is never selected), weights that are neither constant, a temperature that is not positive or not finite,
 * exactly one of idx / val null, an element count of cost or src above 2^31 - 1 (idx and val have fewer than cost). */
#define VDR_WINDOW_VOTE_MAX_SOURCES 8
#define VDR_WINDOW_VOTE_MAX_K 16
#define VDR_WINDOW_VOTE_MAX_CLASSES 64
#define VDR_VOTE_SOFTMAX 0
#define VDR_VOTE_UNIFORM 1
int vdr_op_window_vote(const float* cost, const float* src, int problems, int sources, int gh, int gw, int radius, int k,
                       int n_classes, int weights, float temperature, float* scores, int32_t* labels, int32_t* idx, float* val,
                       void* stream);

/* Thresholded affinity graph of a descriptor map, one bit per pair (csrc/affinity.hip): for each of `pairs` problems the
 * graph B[i, j] = cos(x_i, x_j) > tau over the rows of X_p, without the t x t matrix of scores ever being written.
 *   X_p = [t, d] bf16, rows ldx elements apart, starting at x + p * x_stride (0 allowed).
 * Definition:
 *   ss, rn    = vdr_op_nn_cosine's: rn(v) = 1.0f / fmaxf(sqrtf(ss(v)), 1e-8f), correctly rounded sqrtf and division;
 *   sim(i, j) = dot(x_i, x_j) * (rn(x_i) * rn(x_j)): the two norms are multiplied FIRST (one rounding), then the dot product by
 *               that (one rounding); dot is accumulated in fp32 by bf16 MFMAs in ascending k.  Every step commutes in
 *               (i, j), so sim(i, j) == sim(j, i) bit for bit (vdr_op_nn_cosine's (dot * rn_i) * rn_j does not promise that);
 *   B[i, j]   = sim(i, j) > tau, an fp32 comparison, strict; exclude_diag != 0 clears B[i, i].
 *   bits[p][i][j >> 5] bit (j & 31) = B[i, j]; rows are `pitch` words apart, pitch = ceil(t / 32) rounded up to a multiple of 4
 *   (16-byte rows); the bits of columns >= t and the padding words are written 0.  Every word is written once, by one thread:
 *   no atomics; a problem's bits do not depend on `pairs` or on its position.  Inputs are finite by contract; a zero row has
 *   sim = 0 against everything.
 * work: vdr_affinity_work_bytes(pairs, t) bytes of device scratch (the row norms), 16-byte aligned.
 * Refused before the device is touched: VDR_ERR_UNSUPPORTED for d % 32 != 0; VDR_ERR_INVALID for a null x, work or bits,
 * non-positive pairs, t or d, ldx < d, x_stride < 0, pointers or strides that are not 16-byte aligned, pairs * t above
 * 2^31 - 1, a pitch other than the one above, a NaN tau.
 *
 * vdr_op_bits_matvec: the product of that graph with nv columns,
 *   y[p, i, c] = sum over j with B[i, j] of v[p, j, c],   v, y = [pairs][t][nv] fp32, 1 <= nv <= 8,
 *   degree[p, i] = number of set bits of row i (int32, exact; NULL skips it).
 * Summation order (part of the definition): per row and column 64 partial sums s_0 .. s_63 (the lanes of one wave); s_l adds,
 * starting from 0.0f, the v[j] of the set bits of words l, l + 64, l + 128, ... in ascending word order and ascending bit order
 * within a word; the 64 sums are folded by the xor butterfly s_l += s_(l ^ 32), then ^ 16, 8, 4, 2, 1 (every lane ends with the
 * total).  (The kernel adds 0.0f for a clear bit instead of skipping it: a sum that starts at +0.0f is never -0.0f, so that
 * changes no bit; a non-finite v[j] behind a clear bit stays out.)  Bits of columns >= t are ignored.  The result depends on
 * (t, nv, inputs) only.
 * Refused: VDR_ERR_UNSUPPORTED for nv outside 1 .. 8; VDR_ERR_INVALID for null bits, v or y, non-positive pairs or t, bits not
 * 16-byte aligned, v / y / degree not 4-byte aligned, pairs * t above 2^31 - 1, a wrong pitch. */
size_t vdr_affinity_work_bytes(int pairs, int t);
int vdr_op_affinity_bits(const void* x, int64_t ldx, int64_t x_stride, int t, int pairs, int d, float tau, int exclude_diag,
                         void* work, uint32_t* bits, int pitch, void* stream);
int vdr_op_bits_matvec(const uint32_t* bits, int pitch, int t, int pairs, const float* v, int nv, float* y, int32_t* degree,
                       void* stream);

/* PCA of dense descriptor maps (csrc/pca.hip): the column mean, the centred covariance and the projection on given
 * components.  The eigen-decomposition between the last two is the caller's (vdr.pca.fit: torch.linalg.eigh in float64).
 * Operand, shared by the three entry points: `problems` problems, each `imgs` images of t rows of d channels, R = imgs * t
 *   rows per problem; rows ld elements apart, images image_stride elements apart, image q of problem p is image
 *   p * imgs + q counted from x; in_dtype VDR_BF16 or VDR_F32.  Per-image PCA of a batch B is problems = B, imgs = 1; joint
 *   PCA is problems = 1, imgs = B.  A view into a wider buffer (a key facet inside the qkv activation, ld = 3D) is read in
 *   place.  work: vdr_pca_work_bytes(problems, imgs, t, d) bytes of device scratch, 16-byte aligned, enough for any of the
 *   three.  Rows are cut into chunks of VDR_COV_CHUNK rows; the chunk length is part of the definition, not a launch
 *   heuristic.  No atomics; results are bitwise reproducible, and a problem's result depends neither on `problems` nor on
 *   its position in the batch.
 * vdr_op_col_mean:  mean[p, c] = S / float(R), one IEEE division, S the fp32 sum of column c in this order: inside a chunk
 *   sixteen interleaved sums (rows r, r + 16, r + 32, ... of the chunk, ascending), folded in ascending r; then the chunk sums
 *   in ascending chunk order.                                                                      mean [problems, d] fp32
 * vdr_op_covariance:  z[r, c] = bf16_rn(float(x[r, c]) - mean[p, c]): the subtraction in fp32 BEFORE the one rounding to
 *   bf16, so a map with a large channel mean keeps its variance.  cov[p, c1, c2] = (sum_r z[r, c1] * z[r, c2]) / float(R - 1)
 *   (the n - 1 of sklearn), one IEEE division; the products (exact in fp32) are accumulated in fp32 by bf16 MFMAs over
 *   16 rows at a time, rows ascending within a chunk, and the chunk sums are folded in ascending chunk order.  cov is written
 *   whole and is exactly symmetric (c1 <= c2 is computed, both entries are written from it).  `mean` is an input: any
 *   vector may be passed.  R >= 2.                                                               cov [problems, d, d] fp32
 * vdr_op_pca_project:  proj[p, r, j] = sum_c (float(x[r, c]) - mean[p, c]) * comps[p, j, c], all in fp32 (no bf16 rounding;
 *   separate multiply and add): lane l of 64 sums its channels 8l .. 8l + 7, 512 + 8l .., ... ascending, then the 64 lane
 *   sums are folded by an xor butterfly (distance 32, 16, ... 1).  minmax[p] = (min, max) over the problem's whole [R, k]
 *   block -- one range for all components.  scale != 0: proj = (proj - min) / (max - min), one IEEE subtraction and one
 *   IEEE division per element, when max != min; left as it is otherwise.  k = 1..8.
 *                                      comps [problems, k, d] fp32, proj [problems, R, k] fp32, minmax [problems, 2] fp32
 * Refused before the device is touched: VDR_ERR_UNSUPPORTED for d % 32 != 0, d > 2048, k outside 1..8; VDR_ERR_INVALID for
 * an in_dtype other than the two, null pointers, non-positive problems, imgs, t or d, R < 2 (covariance), ld < d, a negative
 * image_stride, pointers or strides (ld, image_stride) that are not 16-byte aligned, problems * R above 2^31 - 1. */
#define VDR_COV_CHUNK 1024
size_t vdr_pca_work_bytes(int problems, int imgs, int t, int d);
int vdr_op_col_mean(const void* x, int in_dtype, int64_t ld, int64_t image_stride, int problems, int imgs, int t, int d,
                    void* work, float* mean, void* stream);
int vdr_op_covariance(const void* x, int in_dtype, int64_t ld, int64_t image_stride, int problems, int imgs, int t, int d,
                      const float* mean, void* work, float* cov, void* stream);
int vdr_op_pca_project(const void* x, int in_dtype, int64_t ld, int64_t image_stride, int problems, int imgs, int t, int d,
                       const float* mean, const float* comps, int k, int scale, void* work, float* proj, float* minmax,
                       void* stream);
/* The t x t Gram side of the PCA and a top-k eigensolver on the device (csrc/pca.hip, csrc/pca_topk.hip): what
 * vdr.pca.fit(solver="subspace") runs instead of the caller's eigh.  Operand of vdr_op_col_mean_any, vdr_op_gram and
 * vdr_op_pca_back_project: `problems` maps of t rows of d channels (per image only: the operand above with imgs = 1), rows ld and
 * maps image_stride elements apart, in_dtype VDR_BF16 or VDR_F32; d % 32 == 0 with NO upper bound on d.  work:
 * vdr_pca_topk_work_bytes(problems, t, d, k) bytes of device scratch, 16-byte aligned, enough for any op of this block on
 * a t x d operand (k = 8 covers every k) and for vdr_op_sym_topk on matrices of side n = t (side d when d <= 2048 is
 * covered too when the call passes t = max(t, d)).  No atomics; results are bitwise reproducible, and a problem's result depends
 * neither on `problems`, nor on its position in the batch, nor on the grid.
 * vdr_op_col_mean_any:  vdr_op_col_mean's definition, kernels and bits (imgs = 1) at any d.
 * vdr_op_gram:  z[r, c] = bf16_rn(float(x[r, c]) - mean[p, c]), the covariance's centring rule;
 *   gram[p, r1, r2] = (sum_c z[r1, c] * z[r2, c]) / float(t - 1), one IEEE division.  The columns are cut into chunks of
 *   VDR_GRAM_CHUNK columns -- the chunk length is part of the definition --; inside a chunk the products (exact in fp32) are
 *   accumulated in fp32 by bf16 MFMAs over 16 columns at a time, columns ascending; the chunk sums are folded in ascending
 *   chunk order.  gram is written whole and is exactly symmetric (r1 <= r2 is computed, both entries are written from it).
 *   2 <= t <= 4096.  Scratch: one 128 x 128 fp32 tile per (pair of 128-row tiles, chunk).           gram [problems, t, t] fp32
 * vdr_op_pca_back_project:  the step from eigenvectors u of the Gram matrix to components:
 *   c[p, j, :] = sum_r u[p, j, r] * (float(x[r, :]) - mean[p, :]), fp32, separate multiply and add, in col_mean's order:
 *   inside a chunk of VDR_COV_CHUNK rows sixteen interleaved sums (rows r, r + 16, ... ascending) folded in ascending r,
 *   then the chunk sums in ascending chunk order.  Each component is then divided by its norm: the squared norm is
 *   accumulated in float64 (thread i of 256 sums columns i, i + 256, ... ascending, then a binary tree over the threads),
 *   comps = float(double(c) / sqrt(ss)).  A component whose values[p, j] <= 0 or whose norm is 0 is written as zeros.
 *   k = 1..8.                               u [problems, k, t] fp32, values [problems, k] fp32, comps [problems, k, d] fp32
 * vdr_op_sym_topk:  the k largest eigenpairs of symmetric positive semi-definite fp32 matrices a [problems, n, n] (symmetric
 *   by contract: the product is formed as sum_c a[c, r] V[c, :]), n = 2..4096, k = 1..min(8, n).  Block subspace iteration
 *   with a Rayleigh-Ritz step on b = min(16, n) columns; per iteration:
 *     W = A V in fp32 FMAs (no bf16): the contraction is cut into slabs of VDR_TOPK_SLAB rows, inside a slab one FMA chain
 *       per entry, rows ascending; the slab sums are folded in ascending slab order;
 *     H = V^T W in float64, symmetrised; its Ritz pairs (theta_j, y_j) by a cyclic Jacobi (round-robin order; sweeps until no off-diagonal entry exceeds
 *       2^-52 of the largest diagonal one, 10 at most),
 *       sorted descending; residuals res_j = ||W y_j - theta_j V y_j||_2 in float64;
 *     done when res_j <= tol * theta_1 for the k leading pairs, or after max_iter iterations;
 *     else V = orthonormalised columns W y_j / theta_j (rounded to fp32, Gram matrix in float64, Cholesky).  A column whose
 *       Ritz value is not above 2^-40 theta_1 or whose Cholesky pivot is not above 2^-30 of its diagonal is dropped (zero
 *       from then on): a matrix of rank r < k returns k - r zero vectors with value 0.
 *   Start block, fixed: for n <= 16 the first n columns of the identity; else V0[r, c] = +1 / -1 by bit 0 of the hash
 *     h = (r * 0x9E3779B1) ^ (c * 0x85EBCA6B); h ^= h >> 15; h *= 0x2C1B3C6D; h ^= h >> 12; h *= 0x297A2D39; h ^= h >> 15
 *     (uint32 arithmetic; bit set: -1), orthonormalised as above.  A problem's iterates are a property of the problem alone.
 *   Outputs: values [problems, k] fp32 descending; vectors [problems, k, n] fp32, V y_j divided by its float64 norm, the entry of
 *     largest magnitude positive (lowest index on a tie); iters [problems] int32, the iterations (A V products) used;
 *     resid [problems] fp32 = max_j res_j / theta_1 at exit: a problem that ran into max_iter is told by resid > tol.
 *   No host synchronisation: max_iter iterations are enqueued, every launch returns at once for a finished problem.
 *   VDR_TOPK_TOL / VDR_TOPK_MAX_ITER: the defaults of vdr.ops.sym_topk and vdr.pca.fit, measured (profiles/pca_topk_bench.txt).
 *     tol: with tol = 0 the residual stops falling at 3e-8 .. 8.2e-8 of theta_1 on planted spectra of n = 200 .. 4096 (no
 *     growth with n: no fp32 chain is longer than a slab); four times the worst, 3.3e-7.  max_iter: the golden sklearn maps
 *     need 3 - 4 iterations, ViT-B/16 key facets 27 - 42, their log-binned 729 x 13 056 map 73; twice that, 146.
 *     Left out of that rule on purpose: the synthetic white-noise maps of the README's PCA table, whose spectrum does not
 *     fall (80 - 94 iterations at 196 x 768, 142 at 729 x 768, 218 at 3969 x 768, so the rule would give 436 or more): they
 *     run into max_iter at the covariance sizes and vdr.pca.fit decomposes them by eigh, which README reports as losses.
 * Refused before the device is touched: VDR_ERR_UNSUPPORTED for d % 32 != 0, t outside 2..4096 (gram), n outside 2..4096,
 * k outside 1..8 (or above n); VDR_ERR_INVALID for an in_dtype other than the two, null pointers, non-positive problems, t
 * or d, ld < d, a negative image_stride, pointers or strides that are not 16-byte aligned, problems * t above 2^31 - 1, a
 * negative or NaN tol, max_iter < 1. */
#define VDR_GRAM_CHUNK 256
#define VDR_TOPK_SLAB 128
#define VDR_TOPK_TOL 3.3e-7f
#define VDR_TOPK_MAX_ITER 146
size_t vdr_pca_topk_work_bytes(int problems, int t, int d, int k);
int vdr_op_col_mean_any(const void* x, int in_dtype, int64_t ld, int64_t image_stride, int problems, int t, int d, void* work,
                        float* mean, void* stream);
int vdr_op_gram(const void* x, int in_dtype, int64_t ld, int64_t image_stride, int problems, int t, int d, const float* mean,
                void* work, float* gram, void* stream);
int vdr_op_pca_back_project(const void* x, int in_dtype, int64_t ld, int64_t image_stride, int problems, int t, int d,
                            const float* mean, const float* u, const float* values, int k, void* work, float* comps,
                            void* stream);
int vdr_op_sym_topk(const float* a, int problems, int n, int k, float tol, int max_iter, void* work, float* values,
                    float* vectors, int32_t* iters, float* resid, void* stream);
/* Lloyd's k-means over dense descriptor maps (csrc/kmeans.hip): the assignment step and the update step.  The loop, the
 * initialisation and the restarts are the caller's (vdr.kmeans.fit).
 * Operand of both: `problems` problems, each `imgs` images of t rows of d bf16 channels, R = imgs * t rows per problem; rows
 *   ld elements apart, images image_stride elements apart, problems problem_stride elements apart: image q of problem p
 *   starts at x + p * problem_stride + q * image_stride.  problem_stride = imgs * image_stride is the PCA ops' operand;
 *   problem_stride = 0 is one map under `problems` sets of centroids (restarts).  A view into a wider buffer is read in
 *   place.  k = 1..1024 clusters, k <= R; centroids [problems, k, d] fp32.
 *   active: NULL, or [problems] int32 -- a problem whose entry is 0 is skipped by every launch and none of its outputs is
 *   touched (a converged problem in a loop enqueued without host synchronisation).  `active` may be the `changed` array
 *   itself.  work: vdr_kmeans_work_bytes(problems, imgs, t, d, k) bytes of device scratch, 16-byte aligned, enough for
 *   either op.  No atomics; results are bitwise reproducible, and a problem's result depends neither on `problems` nor on
 *   its position in the batch.  Inputs are finite by contract.
 * vdr_op_kmeans_assign:  with x_i the rows and c_j the centroids,
 *   c_hi = bf16_rn(c), c_lo = bf16_rn(c - float(c_hi)) per element (the subtraction is exact; what hi + lo leaves of c is at
 *     most 2^-17 |c|);
 *   s(i, j) = dot(x_i, c_hi_j) + dot(x_i, c_lo_j): ONE fp32 accumulation by bf16 MFMAs (the products are exact in fp32) over
 *     16 channels at a time, channels ascending, per 16 channels the products with c_hi and then those with c_lo;
 *   cc_j = sum_c c_jc^2 of the fp32 centroid, each square rounded to fp32; lane l of 64 sums the channels 8l .. 8l + 7,
 *     512 + 8l .., ... ascending, then the 64 lane sums are folded by an xor butterfly (distance 32, 16, ... 1); xx_i the
 *     same over the row's channels (its squares are exact);
 *   h(i, j) = cc_j - 2 s(i, j), one rounding;  labels[p, i] = argmin_j h(i, j): comparison < on the value, then < on the
 *     index;  min_dist[p, i] = max(xx_i + h(i, label), 0);
 *   inertia[p] = sum_i min_dist[p, i] in col_mean's order (inside a chunk of VDR_COV_CHUNK rows sixteen interleaved sums,
 *     rows r, r + 16, ... ascending, folded in ascending r; then the chunk sums ascending);
 *   changed[p] = the number of rows whose label differs from the value found in labels[p, i] before the call: labels is read
 *     and written, the caller initialises it (to -1: every row counts).
 *   The R x k matrix is never written.  labels [problems, R] int32, min_dist [problems, R] fp32, inertia [problems] fp32,
 *   changed [problems] int32.
 * vdr_op_kmeans_update:  counts[p, j] = the number of rows with labels[p, i] == j (labels outside 0..k-1 are in no cluster);
 *   sum[p, j, :] = sum over those rows of float(x_i), accumulated in fp32 by bf16 MFMAs against a one-hot operand (0 / 1:
 *   exact) over 16 rows at a time, rows ascending within a chunk of VDR_KMEANS_CHUNK rows; the chunk sums are folded in
 *   ascending chunk order.  The chunk length is part of the definition, not a launch heuristic.
 *   centroids[p, j, :] = sum / float(counts), one IEEE division; a cluster with counts == 0 keeps its centroid's bits
 *   (centroids is read and written).                          centroids [problems, k, d] fp32, counts [problems, k] int32
 * Refused before the device is touched: VDR_ERR_UNSUPPORTED for d % 32 != 0 or k outside 1..1024; VDR_ERR_INVALID for null
 * pointers (active excepted), non-positive problems, imgs, t or d, k > R, ld < d, negative strides, pointers or strides
 * (ld, image_stride, problem_stride) that are not 16-byte aligned, problems * R above 2^31 - 1. */
#define VDR_KMEANS_CHUNK 256
size_t vdr_kmeans_work_bytes(int problems, int imgs, int t, int d, int k);
int vdr_op_kmeans_assign(const void* x, int64_t ld, int64_t image_stride, int64_t problem_stride, int problems, int imgs, int t,
                         int d, int k, const float* centroids, const int32_t* active, void* work, int32_t* labels,
                         float* min_dist, float* inertia, int32_t* changed, void* stream);
int vdr_op_kmeans_update(const void* x, int64_t ld, int64_t image_stride, int64_t problem_stride, int problems, int imgs, int t,
                         int d, int k, const int32_t* labels, const int32_t* active, void* work, float* centroids,
                         int32_t* counts, void* stream);
/* Squared Mahalanobis distances of dense descriptor rows under a Gaussian (csrc/mahalanobis.hip): the score side of the
 * Gaussian-of-features anomaly methods (vdr.anomaly).  The fit -- mean, covariance, eigen-decomposition, whitening rows -- is
 * the caller's (vdr.anomaly.whitening).
 * Operand: the k-means ops' -- `problems` problems, each `imgs` images of t rows of d bf16 channels, R = imgs * t rows per
 *   problem; rows ld, images image_stride, problems problem_stride elements apart (0: one map under `problems` models); a view
 *   into a wider buffer is read in place.  The model of problem p: mean + p * mean_stride, [d] fp32, and
 *   whiten + p * whiten_stride, [k][d] fp32 contiguous; a model stride of 0 is one model under every problem.
 *   k = 1..VDR_MAHALANOBIS_MAX_K whitening rows, below, equal to or above d: the op squares whatever rows it is given.
 * For row x_i of problem p:
 *   z = float(x_i) - mean, one fp32 rounding per channel (the subtraction BEFORE any rounding to bf16);
 *   z_hi = bf16_rn(z), z_lo = bf16_rn(z - float(z_hi)) per channel (the subtraction is exact);
 *   for whitening row w_j: w_hi = bf16_rn(w_j), w_lo = bf16_rn(w_j - float(w_hi));
 *   y_j = ONE fp32 accumulation by bf16 MFMAs (the products are exact in fp32) over 16 channels at a time, channels ascending,
 *     per 16 channels the products z_hi.w_hi, then z_hi.w_lo, then z_lo.w_hi; z_lo.w_lo is dropped on purpose (it is below
 *     2^-16 of the leading product, at the level of the fp32 accumulation's own rounding);
 *   d2[p, i] = sum_j y_j * y_j, each square rounded to fp32 before it is added, in this order: 64 partial sums s_(w, l),
 *     w = 0, 1 and l = 0..31, where s_(w, l) adds, starting from 0.0f, the squares of the j with j mod 32 = l and
 *     (j / 64) mod 2 = w in ascending j; T_w = the 32 sums s_(w, .) folded by the xor butterfly s_l += s_(l ^ 1), then ^ 2, 4, 8,
 *     16 (every lane ends with the total); d2 = T_0 + T_1.  The j are counted up to the next multiple of 128 above k - 1: a j >= k
 *     adds +0.0f, which changes no bit.
 *   The order depends on (k, d, inputs) only -- not on `problems`, the problem's position in the batch, R, the grid or a
 *   launch heuristic.  No atomics, no scratch; the R x k matrix of the y is never written.  A non-finite value in row i reaches
 *   d2[p, i] alone; rows past R, whitening rows past k and channels past d are never read.      d2 [problems, R] fp32
 * Refused before the device is touched: VDR_ERR_UNSUPPORTED for d % 32 != 0 or k outside 1..VDR_MAHALANOBIS_MAX_K;
 * VDR_ERR_INVALID for null pointers, non-positive problems, imgs, t or d, ld < d, negative strides, a non-zero mean_stride
 * below d or whiten_stride below k * d, x / mean / whiten or strides (ld, image_stride, problem_stride, mean_stride,
 * whiten_stride) that are not 16-byte aligned, d2 not 4-byte aligned, problems * R above 2^31 - 1. */
#define VDR_MAHALANOBIS_MAX_K 2048
int vdr_op_mahalanobis(const void* x, int64_t ld, int64_t image_stride, int64_t problem_stride, int problems, int imgs, int t,
                       int d, const float* mean, int64_t mean_stride, const float* whiten, int64_t whiten_stride, int k,
                       float* d2, void* stream);
/* Joint bilateral upsampling of a dense descriptor map to pixel resolution, guided by the image the descriptors came from
 * (csrc/upsample.hip; Kopf et al. 2007, the parameter-free filter of FeatUp's JBU up-sampler).
 * Inputs:
 *   F      [batch, gh, gw, C] features, f_dtype VDR_BF16 or VDR_F32 (fp32 is rounded ONCE to bf16 when it is staged; below F means
 *          that bf16 value), read in place: patch (i, j) of image b starts at f + b * image_stride + (i * gw + j) * ld elements.
 *          A key facet inside a qkv activation has ld = 3C.  C % 8 == 0.
 *   G      [batch, Cg, H, W] guide, guide_dtype VDR_F32 or VDR_BF16, contiguous NCHW, Cg = 1..4: the image batch itself.
 *   p, s   patch and stride of the grid, s | p, H = p + (gh - 1) s, W = p + (gw - 1) s.
 *   r      radius 1..3;  cs = 1 / (2 sigma_s^2 s^2), cr = 1 / (2 sigma_r^2): computed by the caller in double and rounded once to
 *          fp32 (sigma = inf gives 0);  m [batch, gh, gw] fp32 confidences >= 0, NULL = 1 everywhere.
 *   box    y0 <= Y < y1, x0 <= X < x1 in pixels, inside the image; out [batch, y1 - y0, x1 - x0, C] channel-last, out_dtype
 *          VDR_BF16 or VDR_F32.
 * vdr_op_guide_lowres (the first launch of vdr_op_upsample_guided; on its own it fills the whole grid):
 *   g_lr[b, g, i, j] = S / float(p * p), one IEEE division, S the fp32 sum, starting from 0.0f, of float(G[b, g, i s + ky, j s + kx])
 *   in ascending (ky, kx) order, ky outer.                                     work = g_lr [batch, Cg, gh, gw] fp32
 *   vdr_op_upsample_guided writes only the g_lr of the patches its box can reach (the nearest patches of the box, r further
 *   each way, inside the grid); the rest of work is not touched.
 * vdr_op_upsample_guided, for pixel (Y, X) of image b:
 *   nearest patch  i0 = clamp(floor_div(2Y + 1 - p + s, 2s), 0, gh - 1), j0 likewise from X: integer arithmetic, floor division
 *     (the numerator can be negative).  p and s of equal parity: no ties; p even and s odd: a tie goes to the upper index.
 *   window         the positions q = (i0 + a, j0 + b), a, b = -r..r, that lie inside the grid; positions outside do not exist
 *     (no clamped duplicates).
 *   weight of q = (i, j), every step ONE fp32 operation (no contraction):
 *     dy = (2Y + 1 - p - 2 s i) / 2, dx likewise from X and j (exact);  ts = -(dy * dy + dx * dx) * cs (the sum is exact);
 *     dist2 = sum over g ascending of d_g * d_g, d_g = float(G[b, g, Y, X]) - g_lr[b, g, i, j], starting from 0.0f;
 *     tr = -dist2 * cr;  t = ts + tr;
 *     w = 0 when t < -64 (no subnormal reaches a weight or its lo half); else w = expf(t) * m[b, i, j] -- expf is the device
 *     math library's (OCML __ocml_exp_f32: documented maximum error 1 ulp), the product one rounding (none when m is NULL).
 *   sum            w_hi = bf16_rn(w), w_lo = bf16_rn(w - float(w_hi)) (the subtraction is exact);
 *     acc[c] = sum over q of (w_hi[q] + w_lo[q]) * F[q, c]: ONE fp32 accumulation by bf16 MFMAs (the products are exact in
 *     fp32) over 16 window slots at a time, slot (a + r)(2r + 1) + (b + r) ascending, per 16 slots the products with w_hi and
 *     then those with w_lo; slots outside the grid and past the window hold zero weights AND zero descriptors (nothing from
 *     outside the map is ever staged: not other columns of a wider buffer, not rows past the grid, not the next image);
 *     Z = sum over q of w[q] (the fp32 w), starting from 0.0f, in ascending (a, b) order, a outer;
 *     out[b, Y - y0, X - x0, c] = acc[c] / Z, one IEEE division, one rounding to out_dtype;  Z == 0: out = F[b, i0, j0, c],
 *     one rounding to out_dtype.
 *   No atomics, no scratch beyond work; bitwise reproducible.  A pixel's bits depend on its own image, the parameters and
 *   (p, s, gh, gw) only -- not on the batch, the position in the batch or the box: the tiles are the cells of the image's patch
 *   grid (the pixels that share a nearest patch), and the output of a box equals that region of the full-image output bit for
 *   bit.  Contract: the features inside the map, the guide and the confidences are finite.
 * work: vdr_upsample_work_bytes(batch, Cg, gh, gw) bytes of device scratch, 16-byte aligned.
 * Refused before the device is touched: VDR_ERR_UNSUPPORTED for a radius outside 1..3 or Cg outside 1..4; VDR_ERR_INVALID for a
 * dtype other than the two, null pointers (m excepted), C % 8 != 0, ld < C, a negative image_stride, features / work / out or
 * strides (ld, image_stride) that are not 16-byte aligned, a guide or m not aligned to its element, non-positive sizes, s not
 * a divisor of p, H, W that do not match (p, s, gh, gw), an empty box or one outside the image, a box of more than 2^31 - 1
 * pixels, negative or non-finite cs / cr.  Device offsets are 64-bit. */
size_t vdr_upsample_work_bytes(int batch, int Cg, int gh, int gw);
int vdr_op_guide_lowres(const void* guide, int guide_dtype, int batch, int Cg, int H, int W, int p, int s, void* work,
                        void* stream);
int vdr_op_upsample_guided(const void* f, int f_dtype, int64_t ld, int64_t image_stride, int batch, int gh, int gw, int C,
                           const void* guide, int guide_dtype, int Cg, int H, int W, int p, int s, int radius, float cs, float cr,
                           const float* conf, int y0, int x0, int y1, int x1, void* work, void* out, int out_dtype, void* stream);
/* ---- measurement ------------------------------------------------------------------------ */

/* Kernel classes timed by the built-in HIP-event profiler. */
typedef enum {
  VDR_K_IM2COL = 0,
  VDR_K_GEMM_PATCH = 1,
  VDR_K_LAYERNORM = 2,
  VDR_K_GEMM_QKV = 3,
  VDR_K_ATTENTION = 4,
  VDR_K_GEMM_PROJ = 5,
  VDR_K_GEMM_FC1 = 6,
  VDR_K_GEMM_FC2 = 7,
  VDR_K_FINAL_LN = 8,
  VDR_K_ASSEMBLE = 9,  /* CLS / register rows, fp32 stream copy, token assembly; the 2-D RoPE launches (vdr_config_ext.rope) */
  VDR_K_CLS_TAIL = 10, /* out-projection, norm2 and MLP of the last block on the CLS rows only (vdr_config.full_last_block) */
  VDR_K_COUNT = 11
} vdr_kernel_class;

/* When enabled, vdr_forward* brackets every launch with hipEventRecord on the
 * caller's stream.  vdr_profile_read synchronises on those events and returns,
 * per class, the summed milliseconds, the launch count and the algorithmic
 * FLOPs and bytes of those launches since the last read / reset. */
int vdr_profile_enable(vdr_handle h, int on);
/* Restrict the event bracketing to the kernel classes whose bit (1 << class) is set (default: all).
 * Timing one class keeps the profiler's cost out of a throughput measurement. */
int vdr_profile_mask(vdr_handle h, uint32_t class_mask);
int vdr_profile_read(vdr_handle h, double* ms, int64_t* launches, double* flops, double* bytes,
                     int n /* = VDR_K_COUNT */);
const char* vdr_kernel_class_name(int k);

#ifdef __cplusplus
}
#endif
#endif /* VDR_H_ */
