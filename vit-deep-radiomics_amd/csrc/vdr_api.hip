// C ABI of libvdr.so (include/vdr.h): handle, weight packing, forward orchestration, profiler.
// Host code only; every kernel lives in one of the other .hip files of this directory, behind the launch functions of
// vdr_kernels.h.
#include <hip/hip_runtime.h>

#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/vdr.h"
#include "knn_map.h"
#include "mask_decoder_pack.h"
#include "mask_stats_map.h"
#include "components_map.h"
#include "edt_map.h"
#include "edt3d_map.h"
#include "local_corr_map.h"
#include "vdr_kernels.h"

using namespace vdr;

namespace {

thread_local std::string g_err;

int round_up(int v, int m) { return (v + m - 1) / m * m; }

// entry points run on the handle's device whatever the caller's current device is, and leave that one current
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    else prev = -1;  // nothing to restore
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- owners: what a handle holds on the device frees itself with the handle (vdr_destroy is `delete`) ------------------------
// Device memory.  Move-only; alloc() is the only allocation of this file and adds the tail pad every buffer carries
// (operand loaders read whole lines past the last element).  Which buffer is (re)allocated when is reserve()'s policy.
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    std::swap(p_, o.p_);
    std::swap(cap_, o.cap_);
    return *this;
  }
  ~DevBuf() { (void)free(); }
  explicit operator bool() const { return p_ != nullptr; }
  void* get() const { return p_; }
  template <class T>
  T* as() const {
    return static_cast<T*>(p_);
  }
  size_t capacity() const { return cap_; }  // bytes asked for (without the pad)
  hipError_t alloc(size_t bytes) {          // (of an empty buffer)
    const hipError_t e = hipMalloc(&p_, bytes + 256);
    if (e != hipSuccess) p_ = nullptr;
    cap_ = p_ ? bytes : 0;
    return e;
  }
  hipError_t free() {
    const hipError_t e = p_ ? hipFree(p_) : hipSuccess;
    p_ = nullptr;
    cap_ = 0;
    return e;
  }

 private:
  void* p_ = nullptr;
  size_t cap_ = 0;
};

// Streams and events: hipStream_t / hipEvent_t are pointers to opaque structs, so unique_ptr owns them as they are
struct StreamDeleter {
  void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
};
struct EventDeleter {
  void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
};
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDeleter>;
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDeleter>;

hipError_t make_stream(Stream& out) {
  hipStream_t s = nullptr;
  const hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  if (e == hipSuccess) out.reset(s);
  return e;
}
hipError_t make_event(Event& out, unsigned flags) {
  hipEvent_t ev = nullptr;
  const hipError_t e = hipEventCreateWithFlags(&ev, flags);
  if (e == hipSuccess) out.reset(ev);
  return e;
}

enum WKind { W_VEC_F32, W_MAT_BF16, W_PATCH_BF16, W_W12_BF16, W_W12_BIAS, W_CONV3_BF16 };

struct WSlot {
  std::string name;
  WKind kind;
  int64_t numel;      // expected fp32 elements from the caller
  int64_t rows, cols; // logical matrix shape for MAT kinds
  DevBuf dev;
  // where resolve() publishes dev: a field of the vdr_model or of one of its layers (typed by the slot's kind)
  const float** dst_f = nullptr;
  const void** dst_v = nullptr;
  bool set = false;
  std::vector<float> host;  // fp32 copy kept until resolve() (LayerNorm folding needs it)
  // SAM encoder built at another input size than its checkpoint: pos_embed (resample = RS_POS) and the rel-pos tables of
  // the global blocks (RS_REL) are also taken at their NATIVE shape -- [1, g0, g0, D] / [2 g0 - 1, 64] -- kept in dev_src,
  // and resampled into dev by resolve().  src_n: g0 / 2 g0 - 1 of the table in dev_src; 0 = dev holds the loaded table.
  int resample = 0;
  int64_t src_n = 0;
  DevBuf dev_src;
};
enum { RS_NONE = 0, RS_POS = 1, RS_REL = 2 };

// the slots (indices into vdr_model::slots) one LayerNorm fold reads: a linear layer's weight and bias, the LayerNorm's
struct FoldIn {
  int w = -1, b = -1, gamma = -1, beta = -1;
};

struct LayerW {
  // the loaded weights (set by resolve() from the slots; a weight the config lacks stays null)
  const float *n1w = nullptr, *n1b = nullptr, *n2w = nullptr, *n2b = nullptr, *bqkv = nullptr, *bproj = nullptr, *b1 = nullptr,
              *b2 = nullptr, *ls1 = nullptr, *ls2 = nullptr;
  const void *wqkv = nullptr, *wproj = nullptr, *w1 = nullptr, *w2 = nullptr;
  const float *relh = nullptr, *relw = nullptr;  // SAM decomposed relative position tables
  DevBuf reltab;  // both tables packed as one [relpos_npad(S)][64] bf16 GEMM operand
  // LayerNorm folded into the consuming GEMM (pre-LN image models): W' = W.diag(gamma) in bf16 (wqkv_f, w1_f),
  // colsum[n] = sum_k W'[n][k] (sqkv, s1), tbias[n] = sum_k beta[k] W[n][k] + b[n] (tqkv, t1)
  FoldIn fold_qkv, fold_fc1;
  DevBuf wqkv_f, w1_f, sqkv, tqkv, s1, t1;
  // fp8 path: MX-fp8 copies (payload, scales) of the qkv / fc1 (w12) / fc2 (w3) weights
  DevBuf qkv_q, qkv_s, w1_q, w1_s, w2_q, w2_s;
};

constexpr int FIN_ROWS = 1 << 16;  // finalisation counters per stream: blocks of >= 64 tile rows, i.e. launches of up to 4 M rows

struct ProfEvent {
  int cls = 0;
  Event a, b;
};

}  // namespace

struct vdr_model {
  vdr_config cfg;
  int device = 0;
  int n_patches = 0, n_tokens = 0, Kp = 0;  // patches / tokens per image at the input size in force
  // vdr_set_input_size: the size in force ((img, img) until the first set) and the position table the forward reads --
  // the loaded pos_embed (pos0) at the native size, else pos_sized [n_tokens, D]: its CLS row and resampled patch rows
  int in_h = 0, in_w = 0;
  // vdr_set_patch_stride: the stride of the patch convolution in force (patch until the first set); the grid in force is
  // grid_h() x grid_w() overlapping patches, n_patches / n_tokens follow it
  int stride = 0;
  const float* pos0 = nullptr;
  DevBuf pos_sized;  // (grows only)
  // vdr_config_ext: register tokens between the CLS row and the patch rows (pos_sized then holds the per-token-row table
  // [CLS position ; n_reg zero rows ; patch positions] at every size, the native one included) and DINOv3's 2-D RoPE
  // (cos / sin [n_patches][head_dim / 2] of the size in force, rebuilt with the position table)
  int n_reg = 0, rope = 0;
  float rope_theta = 100.0f;
  const float* reg = nullptr;
  DevBuf rope_cos, rope_sin;  // (grow only)
  std::vector<WSlot> slots;
  std::map<std::string, int> index;
  std::vector<LayerW> layers;  // sized by vdr_create_ext and never resized: the slots point into it
  const void* w_patch = nullptr;
  const void *w_neck0 = nullptr, *w_neck2 = nullptr;
  const float *neck1w = nullptr, *neck1b = nullptr, *neck3w = nullptr, *neck3b = nullptr;
  const float *b_patch = nullptr, *cls = nullptr, *pos = nullptr, *normw = nullptr, *normb = nullptr,
              *inw = nullptr, *inb = nullptr;
  bool resolved = false;
  bool ln_fuse = false;
  // GEMM weights in the pair-interleaved layout the operand loader wants (gemm_kernels.h), keyed by the row-major
  // device copy they were packed from; built by resolve()
  std::map<const void*, DevBuf> w_il;
  std::string err;
  // internal streams (cfg.streams > 1, or the default split of batch_plan), created by the first forward that forks
  std::vector<Stream> streams;
  Event ev_fork;
  std::vector<Event> ev_join;
  // the default split last worked out (default_split: first part of split_first images, 0 = none, for split_batch images
  // of split_ntok tokens)
  int split_batch = 0, split_ntok = 0, split_first = 0;
  // fp8_cls_bf16: one side stream (+ fork / join events) per stream a forward can run on, created by vdr_finalize; the CLS
  // rows' bf16 MLP of a block runs there under the MX-fp8 GEMMs of the other rows
  std::vector<Stream> aux;
  std::vector<Event> aux_fork, aux_join;
  int cur_aux = 0;  // index of the stream run_blocks is being called for (set by the forward's micro-batch loop)
  // producer-side LayerNorm finalisation (GemmArgs::fin_stats): zeroed counters, one per block of tile rows and per stream
  // a forward can run on (FIN_ROWS each; the kernels leave them zeroed); stats_fresh: the (mean, rstd) buffer of the
  // workspace in use already holds the statistics of the stream's current contents (set by gemm(), taken by ln_consumer())
  DevBuf fin_cnt;
  bool stats_fresh = false;
  // profiler
  bool prof = false;
  uint32_t prof_mask = 0xffffffffu;
  std::vector<ProfEvent> ev_used, ev_free;
  int prof_as = -1;  // >= 0: profiler class every launch is booked under (instead of its own)
  double p_flops[VDR_K_COUNT] = {0}, p_bytes[VDR_K_COUNT] = {0};
  int64_t p_launch[VDR_K_COUNT] = {0};
};

namespace {

#define VDR_TRY(expr, what)                         \
  do {                                              \
    hipError_t _e = (expr);                         \
    if (_e != hipSuccess) return hip_fail(m, _e, what); \
  } while (0)

int hip_fail(vdr_handle h, hipError_t e, const char* what);

// the head dims the attention kernels are built for
bool head_dim_ok(int dh) { return dh == 32 || dh == 64 || dh == 96 || dh == 128; }

// rows in front of the patch rows of an image: the CLS token, then the register tokens
int prefix_rows(const vdr_model* m) { return (m->cfg.has_cls ? 1 : 0) + m->n_reg; }

// the patch grid in force of an image model: Conv2d(kernel = patch, stride = stride) over in_h x in_w pixels
int grid_h(const vdr_model* m) { return (m->in_h - m->cfg.patch) / m->stride + 1; }
int grid_w(const vdr_model* m) { return (m->in_w - m->cfg.patch) / m->stride + 1; }

// input size and patch stride in force, and the patch / token counts that follow from them
void set_geometry(vdr_model* m, int height, int width, int stride) {
  m->in_h = height;
  m->in_w = width;
  m->stride = stride;
  m->n_patches = grid_h(m) * grid_w(m);
  m->n_tokens = m->n_patches + prefix_rows(m);
}

int fail(vdr_handle h, int code, const std::string& msg) {
  if (h) h->err = msg;
  g_err = msg;
  return code;
}

int hip_fail(vdr_handle h, hipError_t e, const char* what) {
  return fail(h, VDR_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// (Re)allocation policies of a handle's buffers.  IF_EMPTY: every load-time copy -- its size is fixed by the config, a
// reload writes into the buffer it has.  GROW: the tables of the input size in force.  REPLACE: a table kept at the shape
// it was loaded with.
enum AllocPolicy { IF_EMPTY, GROW, REPLACE };

int reserve(vdr_model* m, DevBuf& b, size_t bytes, AllocPolicy how, const char* what) {
  if (b && (how == IF_EMPTY || (how == GROW && b.capacity() >= bytes))) return VDR_OK;
  if (b) VDR_TRY(b.free(), ("hipFree(" + std::string(what) + ")").c_str());
  VDR_TRY(b.alloc(bytes), ("hipMalloc(" + std::string(what) + ")").c_str());
  return VDR_OK;
}

// appends the slot of one weight the config wants
WSlot& new_slot(vdr_model* m, const std::string& name, WKind kind, int64_t rows, int64_t cols) {
  m->index[name] = (int)m->slots.size();
  m->slots.emplace_back();
  WSlot& s = m->slots.back();
  s.name = name;
  s.kind = kind;
  s.rows = rows;
  s.cols = cols;
  s.numel = rows * cols;
  return s;
}
// One weight the config wants, and the field of *m (or of m->layers[i]) that resolve() points at its device copy: the fp32
// kinds (vectors, tables) through a const float*, the bf16 kinds (matrices) through a const void*.  Returns the slot's index.
// (The overloads give the typing; the asserts are a developer check only and vanish under NDEBUG.)
bool fp32_kind(WKind k) { return k == W_VEC_F32 || k == W_W12_BIAS; }
int add_slot(vdr_model* m, const std::string& name, WKind kind, int64_t rows, int64_t cols, const float** dst) {
  assert(fp32_kind(kind));
  new_slot(m, name, kind, rows, cols).dst_f = dst;
  return (int)m->slots.size() - 1;
}
int add_slot(vdr_model* m, const std::string& name, WKind kind, int64_t rows, int64_t cols, const void** dst) {
  assert(!fp32_kind(kind));
  new_slot(m, name, kind, rows, cols).dst_v = dst;
  return (int)m->slots.size() - 1;
}

// The only place a weight name is spelled.  The ORDER of the slots is observable (vdr_weight_name).
void build_slots(vdr_model* m) {
  const vdr_config& c = m->cfg;
  const int D = c.dim, F = c.mlp_hidden;
  if (c.patch) {
    add_slot(m, "patch_embed.proj.weight", W_PATCH_BF16, D, (int64_t)c.in_chans * c.patch * c.patch, &m->w_patch);
    add_slot(m, "patch_embed.proj.bias", W_VEC_F32, 1, D, &m->b_patch);
  }
  if (c.has_cls) add_slot(m, "cls_token", W_VEC_F32, 1, D, &m->cls);
  if (m->n_reg) add_slot(m, "register_tokens", W_VEC_F32, m->n_reg, D, &m->reg);
  // (register tokens carry no position: the table is [cls | patches] whatever their number)
  if (c.has_pos) add_slot(m, "pos_embed", W_VEC_F32, m->n_patches + (c.has_cls ? 1 : 0), D, &m->pos0);
  if (c.has_pos && c.window > 0) m->slots.back().resample = RS_POS;
  if (c.input_ln) {
    add_slot(m, "input_norm.weight", W_VEC_F32, 1, D, &m->inw);
    add_slot(m, "input_norm.bias", W_VEC_F32, 1, D, &m->inb);
  }
  for (int i = 0; i < c.layers; ++i) {
    const std::string p = "blocks." + std::to_string(i) + ".";
    LayerW& L = m->layers[i];
    L.fold_qkv.gamma = add_slot(m, p + "norm1.weight", W_VEC_F32, 1, D, &L.n1w);
    L.fold_qkv.beta = add_slot(m, p + "norm1.bias", W_VEC_F32, 1, D, &L.n1b);
    L.fold_qkv.w = add_slot(m, p + "attn.qkv.weight", W_MAT_BF16, 3 * D, D, &L.wqkv);
    L.fold_qkv.b = add_slot(m, p + "attn.qkv.bias", W_VEC_F32, 1, 3 * D, &L.bqkv);
    if (c.window > 0) {
      const int size = ((c.global_mask >> i) & 1) ? c.img / c.patch : c.window;
      const int rs = ((c.global_mask >> i) & 1) ? RS_REL : RS_NONE;  // (window tables do not depend on the grid)
      add_slot(m, p + "attn.rel_pos_h", W_VEC_F32, 2 * size - 1, 64, &L.relh);
      m->slots.back().resample = rs;
      add_slot(m, p + "attn.rel_pos_w", W_VEC_F32, 2 * size - 1, 64, &L.relw);
      m->slots.back().resample = rs;
    }
    add_slot(m, p + "attn.proj.weight", W_MAT_BF16, D, D, &L.wproj);
    add_slot(m, p + "attn.proj.bias", W_VEC_F32, 1, D, &L.bproj);
    if (c.layerscale) add_slot(m, p + "ls1.gamma", W_VEC_F32, 1, D, &L.ls1);
    L.fold_fc1.gamma = add_slot(m, p + "norm2.weight", W_VEC_F32, 1, D, &L.n2w);
    L.fold_fc1.beta = add_slot(m, p + "norm2.bias", W_VEC_F32, 1, D, &L.n2b);
    if (c.act == VDR_ACT_SWIGLU) {
      L.fold_fc1.w = add_slot(m, p + "mlp.w12.weight", W_W12_BF16, 2 * F, D, &L.w1);
      L.fold_fc1.b = add_slot(m, p + "mlp.w12.bias", W_W12_BIAS, 1, 2 * F, &L.b1);
      add_slot(m, p + "mlp.w3.weight", W_MAT_BF16, D, F, &L.w2);
      add_slot(m, p + "mlp.w3.bias", W_VEC_F32, 1, D, &L.b2);
    } else {
      L.fold_fc1.w = add_slot(m, p + "mlp.fc1.weight", W_MAT_BF16, F, D, &L.w1);
      L.fold_fc1.b = add_slot(m, p + "mlp.fc1.bias", W_VEC_F32, 1, F, &L.b1);
      add_slot(m, p + "mlp.fc2.weight", W_MAT_BF16, D, F, &L.w2);
      add_slot(m, p + "mlp.fc2.bias", W_VEC_F32, 1, D, &L.b2);
    }
    if (c.layerscale) add_slot(m, p + "ls2.gamma", W_VEC_F32, 1, D, &L.ls2);
  }
  if (c.pre_ln && c.window == 0) {
    add_slot(m, "norm.weight", W_VEC_F32, 1, D, &m->normw);
    add_slot(m, "norm.bias", W_VEC_F32, 1, D, &m->normb);
  }
  if (c.window > 0) {
    const int C = c.neck_chans;
    add_slot(m, "neck.0.weight", W_MAT_BF16, C, D, &m->w_neck0);
    add_slot(m, "neck.1.weight", W_VEC_F32, 1, C, &m->neck1w);
    add_slot(m, "neck.1.bias", W_VEC_F32, 1, C, &m->neck1b);
    add_slot(m, "neck.2.weight", W_CONV3_BF16, C, (int64_t)C * 9, &m->w_neck2);
    add_slot(m, "neck.3.weight", W_VEC_F32, 1, C, &m->neck3w);
    add_slot(m, "neck.3.bias", W_VEC_F32, 1, C, &m->neck3b);
  }
}

float bf16_to_f32(uint16_t h) {
  uint32_t u = (uint32_t)h << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// tuning knobs are read from the environment in tuning builds only (-DVDR_TUNING, `make tuning`); the shipped library
// has no environment dependence
int env_int(const char* name, int dflt) {
#ifdef VDR_TUNING
  const char* v = getenv(name);
  return v && *v ? atoi(v) : dflt;
#else
  (void)name;
  return dflt;
#endif
}

// (input_ln on an image model -- CLIP's pre_layrnorm -- keeps the fold: the input LayerNorm leaves block 0's row
// statistics itself, launch_ln_rows_stats)
bool ln_fusion_wanted(const vdr_model* m) {
  const vdr_config& c = m->cfg;
  if (c.no_ln_fold || env_int("VDR_LN_FUSE", 1) == 0) return false;
  return c.patch && c.pre_ln && !c.fp8 && (c.dim % 64) == 0;
}

// the fc1 epilogue of the model's MLP activation
int fc1_epilogue(const vdr_config& c) {
  return c.act == VDR_ACT_SWIGLU ? EPI_SWIGLU : c.act == VDR_ACT_QUICK_GELU ? EPI_BIAS_QGELU : c.act == VDR_ACT_GELU_TANH ? EPI_BIAS_TGELU
                                                                                                                            : EPI_BIAS_GELU;
}

// SwiGLU gate pairs: packed row pr of mlp.w12 is source row swiglu_source_row(pr, F) (blocks of 32 x1 rows, then the 32 matching x2 rows:
// the layout of ops.pack_w12 / vdr_set_weight)
int64_t swiglu_source_row(int64_t pr, int64_t F) {
  const int64_t blk = pr / 64, t = pr % 64;
  return t < 32 ? blk * 32 + t : F + blk * 32 + (t - 32);
}

// The host arithmetic of the LayerNorm fold for one linear layer: W' = bf16(gamma . W) [N][K], colsum[n] = float(sum_k
// W'[n][k]) (of the ROUNDED weight: the GEMM multiplies by it), tbias[n] = float(sum_k beta[k] W[n][k] + b[n]); swiglu: rows
// in the gate-pair order (swiglu_source_row).  Shared by the forward (fold_ln) and vdr_ln_fold_weights.
void fold_ln_host(const float* W, const float* b, const float* gam, const float* bet, int64_t N, int64_t K, bool swiglu,
                  uint16_t* wf, float* cs, float* tb) {
  for (int64_t pr = 0; pr < N; ++pr) {
    const int64_t n = swiglu ? swiglu_source_row(pr, N / 2) : pr;
    const float* w = &W[(size_t)n * K];
    double s = 0.0, t = 0.0;
    for (int64_t k = 0; k < K; ++k) {
      const uint16_t h = f32_to_bf16(gam[k] * w[k]);
      wf[(size_t)pr * K + k] = h;
      s += (double)bf16_to_f32(h);
      t += (double)bet[k] * (double)w[k];
    }
    cs[pr] = (float)s;
    tb[pr] = (float)(t + (double)b[n]);
  }
}

// fold_ln_host + upload
int fold_ln(vdr_model* m, const FoldIn& in, int64_t N, int64_t K, bool swiglu, DevBuf& wf_dev, DevBuf& colsum_dev,
            DevBuf& tbias_dev) {
  auto host = [&](int slot) { return m->slots[slot].host.data(); };
  std::vector<uint16_t> wf((size_t)N * K);
  std::vector<float> cs(N), tb(N);
  fold_ln_host(host(in.w), host(in.b), host(in.gamma), host(in.beta), N, K, swiglu, wf.data(), cs.data(), tb.data());
  int rc;
  if ((rc = reserve(m, wf_dev, wf.size() * 2, IF_EMPTY, "folded weight"))) return rc;
  if ((rc = reserve(m, colsum_dev, (size_t)N * 4, IF_EMPTY, "colsum"))) return rc;
  if ((rc = reserve(m, tbias_dev, (size_t)N * 4, IF_EMPTY, "tbias"))) return rc;
  VDR_TRY(hipMemcpy(wf_dev.get(), wf.data(), wf.size() * 2, hipMemcpyHostToDevice), "hipMemcpy(folded weight)");
  VDR_TRY(hipMemcpy(colsum_dev.get(), cs.data(), (size_t)N * 4, hipMemcpyHostToDevice), "hipMemcpy(colsum)");
  VDR_TRY(hipMemcpy(tbias_dev.get(), tb.data(), (size_t)N * 4, hipMemcpyHostToDevice), "hipMemcpy(tbias)");
  return VDR_OK;
}

// DINOv3's RoPE tables for the patch grid of the input size in force (load-time class)
int build_rope_table(vdr_model* m) {
  const vdr_config& c = m->cfg;
  const int half = c.dim / c.heads / 2;
  VDR_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");  // (a forward still in flight may read the old tables)
  const size_t bytes = (size_t)m->n_patches * half * 4;
  int rc;
  if ((rc = reserve(m, m->rope_cos, bytes, GROW, "RoPE table"))) return rc;
  if ((rc = reserve(m, m->rope_sin, bytes, GROW, "RoPE table"))) return rc;
  VDR_TRY(launch_rope2d_table(grid_h(m), grid_w(m), 2 * half, m->rope_theta, m->rope_cos.as<float>(),
                              m->rope_sin.as<float>(), nullptr),
          "rope2d_table");
  VDR_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
  return VDR_OK;
}

// The position tables of the input size and patch stride in force (load-time class: may allocate and synchronise).  Without
// register tokens the native geometry (size img x img at stride patch) reads the loaded pos_embed itself; any other gets
// [CLS row unchanged ; patch rows resampled from the (img / patch)^2 grid to the grid in force].  With register tokens the forward always reads a built table laid out per token row --
// [CLS row ; n_reg zero rows ; patch rows] -- whose patch rows are the loaded ones at the native size (copied: the same
// bits however the handle got there) and the resampled ones elsewhere.  RoPE models (no pos_embed) get their cos / sin tables.
int build_pos_table(vdr_model* m) {
  const vdr_config& c = m->cfg;
  m->pos = m->pos0;
  if (m->rope && c.patch)
    if (int rc = build_rope_table(m)) return rc;
  const bool native = m->in_h == c.img && m->in_w == c.img && m->stride == c.patch;
  if (!c.has_pos || !c.patch || (native && !m->n_reg)) return VDR_OK;
  const int ncls = c.has_cls ? 1 : 0, P = prefix_rows(m), D = c.dim, g0 = c.img / c.patch;
  VDR_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");  // (a forward still in flight, on any stream, may read the old table)
  if (int rc = reserve(m, m->pos_sized, (size_t)m->n_tokens * D * 4, GROW, "pos_embed table")) return rc;
  float* sized = m->pos_sized.as<float>();
  if (ncls) VDR_TRY(hipMemcpy(sized, m->pos0, (size_t)D * 4, hipMemcpyDeviceToDevice), "hipMemcpy(pos_embed CLS row)");
  if (m->n_reg) VDR_TRY(hipMemset(sized + (size_t)ncls * D, 0, (size_t)m->n_reg * D * 4), "hipMemset(register rows)");
  if (native)
    VDR_TRY(hipMemcpy(sized + (size_t)P * D, m->pos0 + (size_t)ncls * D, (size_t)m->n_patches * D * 4, hipMemcpyDeviceToDevice),
            "hipMemcpy(pos_embed patch rows)");
  else
    VDR_TRY(launch_pos_interp(m->pos0 + (size_t)ncls * D, g0, g0, D, sized + (size_t)P * D, grid_h(m), grid_w(m), nullptr),
            "pos_interp");
  VDR_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
  m->pos = sized;
  return VDR_OK;
}

// vdr_set_input_size / vdr_set_patch_stride once their arguments are checked (the caller holds the DeviceGuard): the new
// geometry and its position tables; on failure the geometry in force stays what it was
int change_geometry(vdr_model* m, int height, int width, int stride) {
  const int old_h = m->in_h, old_w = m->in_w, old_s = m->stride;
  set_geometry(m, height, width, stride);
  if (int rc = build_pos_table(m)) {
    set_geometry(m, old_h, old_w, old_s);
    const std::string why = m->err;
    (void)build_pos_table(m);
    return fail(m, rc, why);
  }
  return VDR_OK;
}

// the internal streams vdr_config.streams asks for (what a forward of a given batch runs on: batch_plan)
int configured_streams(const vdr_model* m) { return m->cfg.streams > 1 ? (m->cfg.streams > 8 ? 8 : m->cfg.streams) : 1; }

// the pair-interleaved copy of GEMM weight w [N][K] bf16 (whole-line operand loads, gemm_kernels.h), kept in w_il under w
int interleave(vdr_model* m, const void* w, int N, int K, const char* what_buf, const char* what_launch) {
  auto it = m->w_il.find(w);
  if (it == m->w_il.end()) {
    DevBuf b;
    if (int rc = reserve(m, b, (size_t)N * K * 2, IF_EMPTY, what_buf)) return rc;
    it = m->w_il.emplace(w, std::move(b)).first;
  }
  VDR_TRY(launch_w_interleave(w, it->second.get(), N, K, K, nullptr), what_launch);
  return VDR_OK;
}

// vdr_finalize: everything the forward reads is derived from the loaded weights here (the caller holds the DeviceGuard)
int resolve(vdr_model* m) {
  for (auto& s : m->slots)
    if (!s.set) return fail(m, VDR_ERR_INCOMPLETE, "weight not set: " + s.name);
  if (ln_fusion_wanted(m))
    for (auto& s : m->slots)
      if (s.host.empty())
        return fail(m, VDR_ERR_INCOMPLETE, "weights changed after the first forward: set every weight again (" + s.name + ")");
  const vdr_config& c = m->cfg;
  const int D = c.dim, F = c.mlp_hidden, N1 = c.act == VDR_ACT_SWIGLU ? 2 * F : F;
  int rc;
  for (auto& sl : m->slots) {
    // SAM tables loaded at their native shape: resampled to the handle's grid (segment_anything: bicubic pos_embed as
    // vdr_op_interpolate_pos, get_rel_pos's linear rule as vdr_op_interpolate_rel_pos); the consumers below (rel-pos pack,
    // forward) run later on the same (null) stream and resolve() synchronises before it returns
    if (sl.src_n) {
      if ((rc = reserve(m, sl.dev, (size_t)sl.numel * 4, IF_EMPTY, "resampled table"))) return rc;
      if (sl.resample == RS_POS) {
        const int g = c.img / c.patch;
        VDR_TRY(launch_pos_interp(sl.dev_src.as<float>(), (int)sl.src_n, (int)sl.src_n, c.dim, sl.dev.as<float>(), g, g, nullptr),
                "pos_interp");
      } else {
        VDR_TRY(launch_relpos_interp(sl.dev_src.as<float>(), (int)sl.src_n, 64, sl.dev.as<float>(), (int)sl.rows, nullptr),
                "relpos_interp");
      }
    }
    if (sl.dst_f) *sl.dst_f = sl.dev.as<float>();
    if (sl.dst_v) *sl.dst_v = sl.dev.get();
  }
  if ((rc = build_pos_table(m))) return rc;  // (weights changed: the table of the size in force is rebuilt)
  m->ln_fuse = ln_fusion_wanted(m);
  if (m->ln_fuse) {
    for (LayerW& L : m->layers) {
      if ((rc = fold_ln(m, L.fold_qkv, 3 * D, D, false, L.wqkv_f, L.sqkv, L.tqkv))) return rc;
      if ((rc = fold_ln(m, L.fold_fc1, N1, D, c.act == VDR_ACT_SWIGLU, L.w1_f, L.s1, L.t1))) return rc;
    }
  }
  if (c.fp8) {
    // MX-fp8 copy of a weight; the e4m3 payload goes to the packed (pair-interleaved) layout too: as bytes, [N][K] fp8 is
    // [N][K/2] bf16, and a 32-element bf16 block is one 64-element MX unit
    auto quant = [&](const void* wdev, int N, int K, DevBuf& q, DevBuf& sc) -> int {
      int rc;
      if ((rc = reserve(m, q, (size_t)N * K, IF_EMPTY, "fp8 weight")) ||
          (rc = reserve(m, sc, mx_scale_bytes(N, K), IF_EMPTY, "fp8 weight scales")))
        return rc;
      VDR_TRY(hipMemset(sc.get(), 0, mx_scale_bytes(N, K)), "hipMemset(fp8 weight scales)");
      VDR_TRY(launch_mx_quant(wdev, N, K, K, q.get(), sc.get(), nullptr), "mx_quant(weight)");
      return interleave(m, q.get(), N, K / 2, "interleaved fp8 weight", "w_interleave(fp8)");
    };
    for (LayerW& L : m->layers)
      if ((rc = quant(L.wqkv, 3 * D, D, L.qkv_q, L.qkv_s)) || (rc = quant(L.w1, N1, D, L.w1_q, L.w1_s)) ||
          (rc = quant(L.w2, D, F, L.w2_q, L.w2_s)))
        return rc;
    VDR_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
  }
  if (c.window > 0) {
    const int g = c.img / c.patch;
    for (int i = 0; i < c.layers; ++i) {
      LayerW& L = m->layers[i];
      const int S = (c.global_mask >> i) & 1 ? g : c.window;
      if ((rc = reserve(m, L.reltab, (size_t)relpos_npad(S) * 64 * 2, IF_EMPTY, "rel-pos table"))) return rc;
      VDR_TRY(launch_relpos_pack(L.relh, L.relw, L.reltab.get(), S, nullptr), "relpos_pack");
    }
    VDR_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
  }
  {
    // pair-interleaved copies of every GEMM weight the forward multiplies by
    auto pack = [&](const void* w, int N, int K) -> int {
      if (!w || (N & 1) || (K & 31)) return VDR_OK;
      return interleave(m, w, N, K, "interleaved weight", "w_interleave");
    };
    if (c.patch && (rc = pack(m->w_patch, D, m->Kp))) return rc;
    for (int i = 0; i < c.layers && !c.fp8; ++i) {
      const LayerW& L = m->layers[i];
      if ((rc = pack(L.wqkv, 3 * D, D)) || (rc = pack(L.wqkv_f.get(), 3 * D, D))) return rc;  // (SAM blocks use the unfolded qkv)
      if ((rc = pack(L.wproj, D, D))) return rc;
      if ((rc = pack(L.w1, N1, D)) || (rc = pack(L.w1_f.get(), N1, D))) return rc;
      if ((rc = pack(L.w2, D, F))) return rc;
    }
    if (c.fp8)  // the out-projection stays bf16 on the fp8 path
      for (int i = 0; i < c.layers; ++i)
        if ((rc = pack(m->layers[i].wproj, D, D))) return rc;
    if (c.fp8 && c.fp8_cls_bf16 && c.has_cls) {  // the CLS rows' MLP runs on the bf16 weights
      for (int i = 0; i < c.layers; ++i)
        if ((rc = pack(m->layers[i].w1, N1, D)) || (rc = pack(m->layers[i].w2, D, F))) return rc;
      while (m->aux.size() < (size_t)configured_streams(m)) {  // (the default split leaves fp8 models alone: default_split)
        Stream st;
        Event ea, eb;
        VDR_TRY(make_stream(st), "hipStreamCreate(CLS side stream)");
        VDR_TRY(make_event(ea, hipEventDisableTiming), "hipEventCreate");
        VDR_TRY(make_event(eb, hipEventDisableTiming), "hipEventCreate");
        m->aux.push_back(std::move(st));
        m->aux_fork.push_back(std::move(ea));
        m->aux_join.push_back(std::move(eb));
      }
    }
    if (c.window > 0) {
      if ((rc = pack(m->w_neck0, c.neck_chans, D))) return rc;
      if ((rc = pack(m->w_neck2, c.neck_chans, 9 * c.neck_chans))) return rc;
    }
    VDR_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
  }
  if (!m->fin_cnt) {  // (once per handle: the kernels leave the counters zeroed, so a reload skips the memset and the sync)
    if ((rc = reserve(m, m->fin_cnt, (size_t)8 * FIN_ROWS * 4, IF_EMPTY, "LayerNorm finalisation counters"))) return rc;
    VDR_TRY(hipMemset(m->fin_cnt.get(), 0, (size_t)8 * FIN_ROWS * 4), "hipMemset");
    VDR_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
  }
  for (auto& sl : m->slots) std::vector<float>().swap(sl.host);  // host copies are no longer needed
  m->resolved = true;
  return VDR_OK;
}

// one linear C = epilogue(A . W^T): A [M, K], W [N, K], C [M, N] (EPI_SWIGLU: [M, N / 2]), dense rows, the residual (if
// any) laid out as C; callers set the rest (bias, resid, gamma, strides, row maps, ...) by field
GemmArgs linear(const void* A, const void* W, void* C, int64_t M, int N, int K, int epi) {
  GemmArgs g{};
  g.A = A;
  g.W = W;
  g.C = C;
  g.M = M;
  g.N = N;
  g.K = K;
  g.lda = K;
  g.ldw = K;
  g.ldc = epi == EPI_SWIGLU ? N / 2 : N;
  g.ldr = g.ldc;
  g.omap = identity_map();
  return g;
}

// the weight's pair-interleaved copy, when resolve() made one
void use_interleaved(const vdr_model* m, GemmArgs& g) {
  auto it = m->w_il.find(g.W);
  if (it != m->w_il.end()) {
    g.W = it->second.get();
    g.w_interleaved = 1;
  }
}

// every GEMM of the forward goes through here: the weight is swapped for its interleaved copy
hipError_t launch_gemm_w(vdr_model* m, GemmArgs& g, int epi, int variant, hipStream_t s) {
  use_interleaved(m, g);
  return launch_gemm(g, epi, variant, s);
}

// ---- workspace carving ------------------------------------------------------------------------
struct Carve {
  char *x, *h, *qkv, *o, *u;
  char* hg = nullptr;    // SAM: LN1 output of the global blocks (h holds the windowed, zero-padded order)
  float* rel = nullptr;  // SAM: rel-pos products T[tokens][heads][relpos_npad(S)] (q . every table row)
  char *hs = nullptr, *us = nullptr, *os = nullptr;  // fp8 path: e8m0 scales of the MX activations kept in h, u, o
  char *cls_h = nullptr, *cls_u = nullptr, *cls_x = nullptr;  // fp8_cls_bf16: norm2 / activation / new residual rows of the CLS rows
  float *x32 = nullptr, *xc32 = nullptr;  // resid_fp32: fp32 master copy of the residual stream [Mp, D] / of the compact CLS rows
  float *part, *stats;  // LayerNorm partial sums [D/64][Mp][2] and (mean, rstd) [Mp][2]
  int64_t Mp;
  size_t total;
};

// vdr_config.resid_fp32 applies to the bf16 path of pre-LN image models (plain ViTs: no SAM windows, no fp8)
bool resid_fp32_on(const vdr_config& c) { return c.resid_fp32 && c.pre_ln && c.patch && !c.fp8 && c.window == 0; }

Carve carve(const vdr_model* m, char* base, int mb, int ntok) {
  const vdr_config& c = m->cfg;
  size_t rows = (size_t)mb * ntok;
  size_t rel_floats = 0;
  if (c.window > 0) {
    const size_t g = c.img / c.patch, ws = c.window, nw = (g + ws - 1) / ws;
    const size_t wtok = nw * nw * ws * ws;
    if (wtok > (size_t)ntok) rows = (size_t)mb * wtok;
    const size_t rw = (size_t)mb * wtok * c.heads * relpos_npad((int)ws), rg = (size_t)mb * ntok * c.heads * relpos_npad((int)g);
    rel_floats = rw > rg ? rw : rg;
  }
  const size_t Mp = (size_t)round_up((int)rows, 256) + 256;
  const size_t D = c.dim, F = c.mlp_hidden;
  size_t off = 0;
  Carve w;
  auto take = [&](size_t bytes) {
    char* p = base + off;
    off += align256(bytes);
    return p;
  };
  w.x = take(Mp * D * 2);
  w.h = take(Mp * D * 2);
  w.qkv = take(Mp * 3 * D * 2);
  w.o = take(Mp * D * 2);
  size_t ub = Mp * F * 2;
  if (c.patch) {
    const size_t colb = (size_t)mb * m->n_patches * m->Kp * 2 + 4096;
    if (colb > ub) ub = colb;
  }
  if (c.window > 0) {
    const size_t col3 = (size_t)mb * ntok * 9 * c.neck_chans * 2 + 4096;
    if (col3 > ub) ub = col3;
  }
  w.u = take(ub);
  if (c.window > 0) {
    w.hg = take(Mp * D * 2);
    w.rel = (float*)take(rel_floats * 4 + 256);
  }
  if (c.fp8) {
    w.hs = take(mx_scale_bytes((int64_t)Mp, (int)D));
    w.us = take(mx_scale_bytes((int64_t)Mp, (int)F));
    w.os = take(mx_scale_bytes((int64_t)Mp, (int)D));
    if (c.fp8_cls_bf16 && c.has_cls) {
      const size_t rb = (size_t)round_up(mb, 256);
      w.cls_h = take(rb * D * 2);
      w.cls_u = take(rb * F * 2);
      w.cls_x = take(rb * D * 2);
    }
  }
  if (resid_fp32_on(c)) {
    w.x32 = (float*)take(Mp * D * 4);
    w.xc32 = (float*)take((size_t)round_up(mb, 256) * D * 4);
  }
  w.part = (float*)take((size_t)(D / 64 + 1) * Mp * 8);
  w.stats = (float*)take(Mp * 8);
  w.Mp = (int64_t)Mp;
  w.total = off;
  return w;
}

// fork: the first ns internal streams wait for everything already enqueued on the caller's stream
int fork_streams(vdr_model* m, hipStream_t caller, int ns) {
  if (ns == 1) return VDR_OK;
  while ((int)m->streams.size() < ns) {
    Stream st;
    Event ev;
    if (make_stream(st) != hipSuccess) return VDR_ERR_HIP;
    if (make_event(ev, hipEventDisableTiming) != hipSuccess) return VDR_ERR_HIP;
    m->streams.push_back(std::move(st));
    m->ev_join.push_back(std::move(ev));
  }
  if (!m->ev_fork && make_event(m->ev_fork, hipEventDisableTiming) != hipSuccess) return VDR_ERR_HIP;
  if (hipEventRecord(m->ev_fork.get(), caller) != hipSuccess) return VDR_ERR_HIP;
  for (int i = 0; i < ns; ++i)
    if (hipStreamWaitEvent(m->streams[i].get(), m->ev_fork.get(), 0) != hipSuccess) return VDR_ERR_HIP;
  return VDR_OK;
}

// join: the caller's stream waits for the first ns internal streams
int join_streams(vdr_model* m, hipStream_t caller, int ns) {
  if (ns == 1) return VDR_OK;
  for (int i = 0; i < ns; ++i) {
    if (hipEventRecord(m->ev_join[i].get(), m->streams[i].get()) != hipSuccess) return VDR_ERR_HIP;
    if (hipStreamWaitEvent(caller, m->ev_join[i].get(), 0) != hipSuccess) return VDR_ERR_HIP;
  }
  return VDR_OK;
}

// ---- profiler -----------------------------------------------------------------------------------
struct Scope {  // (m = nullptr: an op entry point, nothing is booked)
  vdr_model* m;
  hipStream_t s;
  ProfEvent e;
  bool on;
  Scope(vdr_model* m_, hipStream_t s_, int cls, double flops, double bytes) : m(m_), s(s_) {
    on = m && m->prof;
    if (!on) return;
    if (m->prof_as >= 0) cls = m->prof_as;  // (block_tail_cls: its small launches are one class of their own)
    on = (m->prof_mask >> cls) & 1u;
    if (!on) return;
    if (!m->ev_free.empty()) {
      e = std::move(m->ev_free.back());
      m->ev_free.pop_back();
    } else {
      (void)make_event(e.a, hipEventDefault);
      (void)make_event(e.b, hipEventDefault);
    }
    e.cls = cls;
    m->p_flops[cls] += flops;
    m->p_bytes[cls] += bytes;
    m->p_launch[cls] += 1;
    hipEventRecord(e.a.get(), s);
  }
  ~Scope() {
    if (!on) return;
    hipEventRecord(e.b.get(), s);
    m->ev_used.push_back(std::move(e));
  }
};

// questions about a tile variant of launch_gemm: lookups in the one table of them (TILE_VARIANTS, vdr_kernels.h)
bool variant_is(int v, TileFamily f) { const TileVariant* r = tile_variant(v); return r && r->family == f; }
bool ring4_variant(int v) { return variant_is(v, TILE_RING4); }
bool ring4_big_variant(int v) { return ring4_variant(v) && tile_variant(v)->bm() >= 128; }  // the forward gives the patch gather and the in-GEMM statistics to these only
// the consumers of the LayerNorm fold that finalise the producers' partials themselves (GemmArgs::ln_cpart)
bool ln_cpart_variant(int v) { return variant_is(v, TILE_RING3) || ring4_big_variant(v); }

// tile configuration per GEMM class; VDR_GEMM_VARIANT overrides all of them (tuning aid)
int gemm_variant_for(int cls, int64_t M = 1 << 30, int N = 1 << 30) {
  VDR_KNOB int forced = env_int("VDR_GEMM_VARIANT", -1);
  if (forced >= 0) return forced;
  // small problems (a single 1024^2 SAM slice is M = 4096): fewer 128x256 tiles than CUs -> 128x128 tiles
  // (measured, MedSAM batch 1: fc2 0.72 -> 0.57 ms, proj 0.35 -> 0.31 ms per forward)
  if (cls != VDR_K_GEMM_QKV && ((M + 127) / 128) * ((N + 255) / 256) < 256) {
    VDR_KNOB int small = env_int("VDR_GEMM_VARIANT_SMALL", -1);
    if (small >= 0) return small;
    // ring4 128x128 tiles (variant 28).  Measured at M = 4096 / 4900 (one MedSAM slice), interleaved rounds: against
    // ring3 128x128 (24) proj 18.8 -> 17.7 us, fc2 43.9 -> 41.0 us.  Variant 25 (the K loop split across two wave groups
    // of the workgroup) is faster still (16.5 / 37.1 us) but sums K in a different order than the big-batch kernels,
    // so a row would no longer be bitwise independent of the batch it travels in: tuning builds only
    // (VDR_GEMM_VARIANT_SMALL=25), the default keeps rows batch-invariant.
    return 28;
  }
  // measured per shape at M = 50432 (tools/kbench.py): 16 waves per CU with 64-register accumulators
  // (wave tile 64x64) beat 8 waves with 128-register accumulators on every shape
  // per-class override for tuning: VDR_GEMM_VARIANT_QKV / _PROJ / _FC1 / _FC2
  VDR_KNOB int o_qkv = env_int("VDR_GEMM_VARIANT_QKV", -1), o_proj = env_int("VDR_GEMM_VARIANT_PROJ", -1),
                   o_fc1 = env_int("VDR_GEMM_VARIANT_FC1", -1), o_fc2 = env_int("VDR_GEMM_VARIANT_FC2", -1);
  const int o = cls == VDR_K_GEMM_QKV ? o_qkv : cls == VDR_K_GEMM_PROJ ? o_proj : cls == VDR_K_GEMM_FC1 ? o_fc1
                : cls == VDR_K_GEMM_FC2 ? o_fc2 : -1;
  if (o >= 0) return o;
  // ring4 (whole-line operand staging: packed weights + 64-deep activation pieces), 128x256 tile, 8 waves, two
  // workgroups per CU.  Measured at M = 50432, interleaved rounds in one process, weights packed in both arms
  // (tools/kbench.py, alternating order): against ring3 128x256 qkv 0.181 -> 0.176 ms, proj 0.086 -> 0.078, fc1
  // 0.267 -> 0.257, fc2 0.246 -> 0.230; the 256x256 forms (ring3 23, ring4 27) lose on every shape.
  return 26;
}

// im2col-free patchify (GemmArgs::patch_p): bf16 NCHW images, 16-byte aligned, patch side 8 / 16 / 32, a ring4 tile variant
bool patch_gather_ok(int in_dtype, int patch, int variant, const void* images) {
  return in_dtype == VDR_BF16 && (patch == 8 || patch == 16 || patch == 32) && ring4_big_variant(variant) &&
         ((uintptr_t)images & 15) == 0;
}

// The patch-embedding GEMM of `batch` images [batch, chans, H, W] at patch stride `stride` (p: no overlap) -> C rows omap(r),
// r < batch * gh * gw with gh x gw = ((H - p) / stride + 1) x ((W - p) / stride + 1), token i of an image being patch
// (i / gw, i % gw): at stride p bf16 images with a patch side of 8 / 16 / 32 on a SQUARE grid are gathered
// 16-byte runs at a time by the GEMM's operand loader straight from NCHW (ring4 tile variants: no col buffer, no im2col
// launch); fp32 images (the loader is an LDS-DMA: it cannot convert), p = 14 (runs of 14 pixels are not 16-byte chunks)
// and rectangular grids (the loader splits a row by one grid side) go through im2col into `col`, launched here, and so does
// every stride below p (the overlapping im2col of patch_stride.hip).  Fills
// *g (the caller adds bias, pos, omap and what else differs) and *variant.
hipError_t patch_gemm(vdr_model* m, hipStream_t s, const void* images, int in_dtype, void* col, const void* W, void* C,
                      int batch, int chans, int H, int Wd, int p, int stride, int D, GemmArgs* g, int* variant) {
  const int n = ((H - p) / stride + 1) * ((Wd - p) / stride + 1), Kp = round_up(chans * p * p, 64);
  *variant = gemm_variant_for(VDR_K_GEMM_PATCH, (int64_t)batch * n, D);
  const bool fused = stride == p && H == Wd && patch_gather_ok(in_dtype, p, *variant, images);
  *g = linear(fused ? images : col, W, C, (int64_t)batch * n, D, Kp, EPI_PATCH);
  if (fused) {
    g->patch_p = p;
    g->patch_g = H / p;
    g->patch_C = chans;
    return hipSuccess;
  }
  const size_t in_es = in_dtype == VDR_BF16 ? 2 : 4;
  Scope sc(m, s, VDR_K_IM2COL, 0.0, (double)batch * chans * H * Wd * in_es + 2.0 * batch * n * Kp);
  if (stride != p) return launch_im2col_strided(images, in_dtype == VDR_BF16, col, batch, chans, H, Wd, p, stride, Kp, s);
  return launch_im2col(images, in_dtype == VDR_BF16, col, batch, chans, H, Wd, p, Kp, s);
}

#ifndef VDR_GEMM_8P_DEFAULT
#define VDR_GEMM_8P_DEFAULT 3  // qkv + fc1, measured in the forward per launch: qkv 172 -> 147 us; fc1 (erf-GELU) 257 -> 247 once the two wave sets finish a half tile in the same slot (gemm_8p.hip), ViT-L/14@336 fc1 7.62 -> 6.89 ms per step
#endif

struct LnFold {
  const float* stats = nullptr;   // consumer: (mean, rstd) per row
  const float* colsum = nullptr;  // consumer: column sums of the folded weight
  float* part = nullptr;          // producer: partial sums out
  int64_t part_stride = 0;
  const float* cpart = nullptr;   // consumer: the producers' partials, finalised inside the GEMM (instead of stats)
  int groups = 0;
  int64_t cstride = 0;
  float eps = 0.0f;
  float* fin_stats = nullptr;     // producer: finalise the statistics of the rows it completes here (see finalize_rows_if_last)
  uint32_t* fin_cnt = nullptr;    //   with these zeroed counters, one per 64 rows (left zeroed)
};

// LnFold -> GemmArgs: the one place the fold's fields are filled, for the forward's gemm() and the vdr_op_linear_ln_*
// entry points alike
void set_ln_fold(GemmArgs& g, const LnFold& ln) {
  g.ln_stats = ln.stats;
  g.colsum = ln.colsum;
  g.ln_part = ln.part;
  g.part_stride = ln.part_stride;
  g.ln_cpart = ln.cpart;
  g.ln_groups = ln.groups;
  g.ln_cstride = ln.cstride;
  g.ln_eps = ln.eps;
  if (ln.fin_stats && ln.fin_cnt) {
    g.fin_stats = ln.fin_stats;
    g.fin_cnt = ln.fin_cnt;
    g.fin_eps = ln.eps;
  }
}

// which GEMM classes take tile variant 31 when the launch is eligible (gemm_8p_eligible): measured per class in the
// forward; tuning builds: VDR_GEMM_8P = bit mask (1 qkv, 2 fc1), -1 = the default
bool use_8p(int cls) {
  VDR_KNOB int mask_env = env_int("VDR_GEMM_8P", -1);
  const int mask = mask_env >= 0 ? mask_env : VDR_GEMM_8P_DEFAULT;
  return (cls == VDR_K_GEMM_QKV && (mask & 1)) || (cls == VDR_K_GEMM_FC1 && (mask & 2));
}

// whether tile variant 31 takes a launch of this class and shape: gemm() asks this and then gemm_8p_eligible of the
// launch itself; ln_stats_in_gemm asks this alone
bool wants_8p(int cls, int64_t M, int N) { return use_8p(cls) && gemm_8p_shape_ok(M, N); }

// Tile variant 31 (gemm_8p.hip) for the write-once linears of large launches (plain weight layout).  The workspace
// buffers A points into hold Mp >= M + 256 rows, so a ragged last 256-row tile reads rows that exist; they are never stored.
bool takes_8p(int cls, const GemmArgs& g, int epi) {
  return g.lda == g.K && g.a_rows > 0 && wants_8p(cls, g.M, g.N) && gemm_8p_eligible(g, epi);
}

// Where the (sum, sumsq) partials of the residual stream become (mean, rstd): inside the consuming GEMM when it runs
// a ring3 variant (22-24; every workgroup finalises its own rows in LDS while its ring fills: no launch), otherwise by
// ln_finalize_kernel ahead of it.  Same arithmetic either way: results are bitwise equal.  Measured (same box,
// alternating runs): the fetch of the partials adds about a microsecond to every tile's prologue, so it pays where a
// launch is a handful of tile rounds (MedSAM batch 1: 2.694 -> 2.669 ms, batch 4: 6.606 -> 6.588) and costs where it
// is many (ViT-B batch 256: qkv +3 %, fc1 +4 % against 0.15 ms of ln_finalize launches: 12.15 -> 12.19 ms): taken
// for launches of at most 2048 tiles.  VDR_LN_IN_GEMM=0 / 1 forces the separate kernel / the in-GEMM form.
bool ln_stats_in_gemm(int cls, int64_t M, int N, int groups) {
  VDR_KNOB int mode = env_int("VDR_LN_IN_GEMM", -1);
  const int v = gemm_variant_for(cls, M, N);
  if (mode == 0 || groups > 16 || !ln_cpart_variant(v)) return false;
  if (mode == 1) return true;
  // (a launch the 8-phase kernel takes reads finalised statistics: it has no in-GEMM finalisation)
  // (known quirk: predicted from the shape alone, so a launch variant 31 refuses -- SwiGLU fc1 -- gets no finalisation either)
  if (wants_8p(cls, M, N)) return false;
  return ((M + 127) / 128) * ((N + 255) / 256) <= 2048;
}

// consumer side of the fold for one GEMM: hands it the partials, or finalises the statistics ahead of it
int ln_consumer(vdr_model* m, hipStream_t s, int cls, int64_t M, int N, int D, const Carve& w, LnFold* cons) {
  const int groups = D / 64;
  if (ln_stats_in_gemm(cls, M, N, groups)) {
    cons->stats = nullptr;
    cons->cpart = w.part;
    cons->groups = groups;
    cons->cstride = w.Mp;
    cons->eps = m->cfg.ln_eps;
    m->stats_fresh = false;
    return VDR_OK;
  }
  if (!m->stats_fresh) {  // (otherwise the residual GEMM that wrote the stream finalised its rows' statistics itself)
    Scope sc(m, s, VDR_K_LAYERNORM, 0.0, (double)M * (groups + 1) * 8);
    VDR_TRY(launch_ln_finalize(w.part, groups, w.Mp, w.stats, M, D, m->cfg.ln_eps, s), "ln_finalize");
  }
  m->stats_fresh = false;
  cons->cpart = nullptr;
  cons->stats = w.stats;
  return VDR_OK;
}

// Every GEMM of the forward but the SAM out-projection: g is the launch as linear() and the caller describe it (a_rows:
// rows of A / of the fold's row statistics that are readable, the workspace's Mp; 0 = unknown), ln the LayerNorm fold.
// Books the launch, picks the tile variant and, for a producer of partials, who finalises them.
int gemm(vdr_model* m, hipStream_t s, int cls, GemmArgs g, int epi, const LnFold& ln = LnFold()) {
  const int variant = gemm_variant_for(cls, g.M, g.N);
  // a producer of LayerNorm partials on a ring4 tile variant also finalises them (finalize_rows_if_last): the consumer's
  // ln_finalize launch is not needed then (ln_consumer takes m->stats_fresh)
  const bool fin = ln.fin_stats && ln.part && m->fin_cnt && m->cfg.ln_fin_fused && ring4_variant(variant) && epi == EPI_BIAS_RESID &&
                   (g.M + 63) / 64 <= FIN_ROWS;
  LnFold lnf = ln;
  lnf.fin_cnt = fin ? m->fin_cnt.as<uint32_t>() + (size_t)m->cur_aux * FIN_ROWS : nullptr;
  if (fin) lnf.eps = m->cfg.ln_eps;
  set_ln_fold(g, lnf);
  const double outw = epi == EPI_SWIGLU ? g.N / 2 : g.N;
  Scope sc(m, s, cls, 2.0 * g.M * g.N * g.K,
           2.0 * ((double)g.M * g.K + (double)g.N * g.K + (double)g.M * outw * (g.resid32 ? 5 : g.resid ? 2 : 1)));  // (fp32 in + fp32 out + bf16 out)
  if (takes_8p(cls, g, epi))
    VDR_TRY(launch_gemm(g, epi, VARIANT_8P, s), "gemm_8p");
  else
    VDR_TRY(launch_gemm_w(m, g, epi, variant, s), "gemm");
  if (ln.part) m->stats_fresh = fin;
  return VDR_OK;
}

// one LayerNorm launch of the forward, booked under kernel class `cls`
int layernorm(vdr_model* m, hipStream_t s, int cls, const LnArgs& a) {
  Scope sc(m, s, cls, 0.0, (double)a.rows * a.D * ((a.in_bf16 ? 2 : 4) + (a.out_bf16 ? 2 : 4)));
  VDR_TRY(launch_layernorm(a, s), "layernorm");
  return VDR_OK;
}

int layernorm(vdr_model* m, hipStream_t s, int cls, const void* x, int in_bf16, void* y, int out_bf16,
              const float* gw, const float* gb, int64_t rows, RowMap imap, const float* clsrc = nullptr,
              int cls_period = 0, int width = 0, int64_t ldy = 0) {
  LnArgs a{};
  a.x = x;
  a.in_bf16 = in_bf16;
  a.y = y;
  a.out_bf16 = out_bf16;
  a.gamma = gw;
  a.beta = gb;
  a.rows = rows;
  a.D = width ? width : m->cfg.dim;
  a.eps = m->cfg.ln_eps;
  a.imap = imap;
  a.omap = identity_map();
  a.cls = clsrc;
  a.cls_period = cls_period;
  a.ldy = ldy;
  return layernorm(m, s, cls, a);
}

// tile configuration of the MX-fp8 GEMM per class and shape (VDR_MX_VARIANT overrides)
int mx_variant_for(int cls, int64_t M, int N) {
  VDR_KNOB int forced = env_int("VDR_MX_VARIANT", -1);
  if (forced >= 0) return forced;
  if (((M + 127) / 128) * ((N + 255) / 256) < 256) return 2;  // small problem: 128x128 tiles
  if (cls == VDR_K_GEMM_QKV) return 0;
  return M >= 16384 ? 0 : 1;  // measured (tools/mx_bench.py): 256x256 tiles win at ViT-g's M = 8224
}

// one linear on the block-scaled fp8 MFMA: MX operands (aq, as) x (wq, wsc); cs != NULL -> MX output
int gemm_mx(vdr_model* m, hipStream_t s, int cls, const void* aq, const void* as, const void* wq, const void* wsc,
            const float* bias, const void* resid, const float* gamma, void* C, void* cs, int64_t M, int N, int K, int epi) {
  GemmArgs g = linear(aq, wq, C, M, N, K, epi);
  g.a_scale = as;
  g.w_scale = wsc;
  g.bias = bias;
  g.resid = resid;
  g.gamma = gamma;
  g.c_scale = cs;
  const double outb = cs ? 1.0 : 2.0;
  Scope sc(m, s, cls, 2.0 * M * N * K, (double)M * K + (double)N * K + (double)M * g.ldc * (resid ? 2 * outb : outb));
  VDR_KNOB int packed = env_int("VDR_MX_PACKED", 1);  // (tuning builds: 0 = the row-major payload, for A/B)
  if (packed) use_interleaved(m, g);
  VDR_TRY(launch_gemm_mx(g, epi, mx_variant_for(cls, M, N), s), "gemm_mx");
  return VDR_OK;
}

// ---- the transformer block --------------------------------------------------------------------------------------------
// How a model's linears take their LayerNorm and their operands.  Chosen once per forward (block_path); the two steps of
// a block that differ between the paths are BlockSteps::norm_linear and BlockSteps::resid_linear, everything else -- the
// block loop of run_blocks, the CLS tail, the CLS rows' bf16 MLP, the MLP half of a SAM block -- is written once over them.
enum BlockPath {
  // BASELINE config 5: qkv / fc1 / fc2 on the block-scaled fp8 MFMA.  LayerNorm writes its output as MX-fp8 (the qkv / fc1
  // operand), the attention kernel and the fc1 epilogue write theirs as MX-fp8 (the proj / fc2 operands); the residual
  // stream and the attention arithmetic stay bf16 / fp32.
  PATH_MX,
  // LayerNorm never materialised: producers leave (sum, sumsq) partials, a tiny kernel turns them into (mean, rstd), the
  // consuming GEMM applies them in its epilogue (weights pre-multiplied by gamma).
  PATH_FOLD,
  // A LayerNorm kernel in front of the linear (pre-LN), or -- post-LN, nn.TransformerEncoderLayer with norm_first=False:
  // x = LN1(x + SA(x)); x = LN2(x + FF(x)) -- the linears read the stream itself and the caller runs the LayerNorms.
  PATH_EXPLICIT
};

BlockPath block_path(const vdr_model* m) { return m->cfg.fp8 ? PATH_MX : (m->cfg.pre_ln && m->ln_fuse) ? PATH_FOLD : PATH_EXPLICIT; }

// Rows of the residual stream as a step reads or writes them: row r is bf16 row r * step of x (step 0: dense rows; ntok:
// the CLS row of every image) and, under resid_fp32, of the fp32 master copy x32 (else null)
struct Rows {
  void* x;
  float* x32;
  int step;
};

struct BlockSteps {
  vdr_model* m;
  hipStream_t s;
  const Carve& w;
  const LayerW& L;
  BlockPath path;

  // LayerNorm (norm1 / norm2) of M rows of the stream, then the linear that reads it (qkv / fc1) into `out`.  h: where the
  // normalised rows go on the paths that materialise them (MX: the payload, its scales in w.hs); a_rows: as gemm() takes
  // it.  Strided rows (in.step) are read by the explicit form only.
  int norm_linear(bool fc1, int64_t M, Rows in, char* h, void* out, int64_t a_rows) const {
    const vdr_config& c = m->cfg;
    const int D = c.dim, cls = fc1 ? VDR_K_GEMM_FC1 : VDR_K_GEMM_QKV, epi = fc1 ? fc1_epilogue(c) : EPI_BIAS;
    const int N = !fc1 ? 3 * D : epi == EPI_SWIGLU ? 2 * c.mlp_hidden : c.mlp_hidden;
    const float *nw = fc1 ? L.n2w : L.n1w, *nb = fc1 ? L.n2b : L.n1b;
    int rc;
    if (path == PATH_MX) {
      {
        Scope sc(m, s, VDR_K_LAYERNORM, 0.0, (double)M * D * 3);  // (own block: the profiler bracket must close before the GEMM)
        VDR_TRY(launch_ln_mx(in.x, nw, nb, c.ln_eps, M, D, h, w.hs, s), "layernorm_mx");
      }
      return gemm_mx(m, s, cls, h, w.hs, (fc1 ? L.w1_q : L.qkv_q).get(), (fc1 ? L.w1_s : L.qkv_s).get(), fc1 ? L.b1 : L.bqkv, nullptr, nullptr, out,
                     fc1 ? w.us : nullptr, M, N, D, epi);
    }
    GemmArgs g;
    LnFold cons;
    if (path == PATH_FOLD) {
      if ((rc = ln_consumer(m, s, cls, M, N, D, w, &cons))) return rc;
      cons.colsum = (fc1 ? L.s1 : L.sqkv).as<float>();
      g = linear(in.x, (fc1 ? L.w1_f : L.wqkv_f).get(), out, M, N, D, epi);
      g.bias = (fc1 ? L.t1 : L.tqkv).as<float>();
    } else {
      // (resid_fp32: the explicit LayerNorm reads the fp32 master copy of the stream)
      if (c.pre_ln && (rc = layernorm(m, s, VDR_K_LAYERNORM, in.x32 ? (const void*)in.x32 : in.x, !in.x32, h, 1, nw, nb, M,
                                      in.step ? RowMap{1, in.step, 0} : identity_map())))
        return rc;
      g = linear(c.pre_ln ? h : in.x, fc1 ? L.w1 : L.wqkv, out, M, N, D, epi);
      g.bias = fc1 ? L.b1 : L.bqkv;
    }
    g.a_rows = a_rows;
    return gemm(m, s, cls, g, epi, cons);
  }

  // The residual linears (proj / fc2): out = in + gamma * (A . W^T + bias) over M rows, A's rows lda elements apart (0:
  // dense); in place, into compact rows, or (post-LN) into the input of the LayerNorm behind it.  prod: the fold's
  // producer side, where a folded consumer reads these rows next (else null).
  int resid_linear(bool fc2, int64_t M, const void* A, int64_t lda, Rows in, Rows out, const LnFold* prod) const {
    const vdr_config& c = m->cfg;
    const int D = c.dim, K = fc2 ? c.mlp_hidden : D, cls = fc2 ? VDR_K_GEMM_FC2 : VDR_K_GEMM_PROJ;
    const float* gamma = fc2 ? L.ls2 : L.ls1;  // (LayerScale; null without)
    if (path == PATH_MX && fc2)
      return gemm_mx(m, s, cls, A, w.us, L.w2_q.get(), L.w2_s.get(), L.b2, in.x, gamma, out.x, nullptr, M, D, K, EPI_BIAS_RESID);
    // (the out-projection stays bf16 on the MX path: quantising it too measured 0.987 row cosine at 40 blocks, gate 0.99)
    GemmArgs g = linear(A, fc2 ? L.w2 : L.wproj, out.x, M, D, K, EPI_BIAS_RESID);
    g.bias = fc2 ? L.b2 : L.bproj;
    g.resid = in.x;
    g.gamma = gamma;
    g.resid32 = in.x32;
    g.C32 = out.x32;
    if (lda) g.lda = lda;
    if (in.step) g.ldr = (int64_t)in.step * D;
    return gemm(m, s, cls, g, EPI_BIAS_RESID, prod ? *prod : LnFold());
  }
};

struct BookAs {  // the profiler books these launches as VDR_K_CLS_TAIL, so that gemm_proj / fc1 / fc2 stay classes of
  vdr_model* m;  // identical full-size launches (their averages are what the rocprofv3 summaries are compared with)
  explicit BookAs(vdr_model* m_) : m(m_) { m->prof_as = VDR_K_CLS_TAIL; }
  ~BookAs() { m->prof_as = -1; }
};

// vdr_config.fp8_cls_bf16: norm2 -> fc1 / w12 -> activation -> fc2 / w3 + residual of the CLS rows (row b * ntok of the
// residual stream) on the bf16 weights, enqueued on `ax`; leaves the rows' new residual values in w.cls_x [mb, D].  Reads
// the residual stream as it is after the out-projection; the caller puts w.cls_x back once the MX-fp8 MLP of every row has
// written w.x.  Same kernels and per-row arithmetic as the CLS tail of the last block (block_tail_cls on the explicit
// path): a row's bits do not depend on which of the two computed it.
int cls_mlp_bf16(vdr_model* m, hipStream_t ax, const Carve& w, const LayerW& L, int mb, int ntok) {
  BookAs book(m);
  const BlockSteps b{m, ax, w, L, PATH_EXPLICIT};
  const Rows cls_rows{w.x, nullptr, ntok};
  if (int rc = b.norm_linear(true, mb, cls_rows, w.cls_h, w.cls_u, 0)) return rc;
  return b.resid_linear(true, mb, w.cls_u, 0, cls_rows, Rows{w.cls_x, nullptr, 0}, nullptr);
}

// CLS-only tail of the LAST block (VDR_OUT_CLS: `model(x) -> (logits, cls)`, models_archs.py:24-29 -- the reference
// computes every token of the last block and then keeps x[:, 0]).  After the last attention nothing mixes rows any
// more: out-projection, norm2, MLP and the final norm are row-wise, so the [mb] CLS rows are all that reaches the output.
// They are gathered by the out-projection itself (A and the residual are read with a row stride of ntok * D, the
// result goes to a compact [mb, D] buffer -- the head of w.h, which no later kernel of this forward reads) and the MLP
// runs on mb rows instead of mb * ntok.  Same kernels, same per-row arithmetic: the CLS features are bitwise those of
// the full block (test_cls_rows_only_last_block_bitwise).  vdr_config.full_last_block = 1 keeps every row.
int block_tail_cls(vdr_model* m, hipStream_t s, const Carve& w, const LayerW& L, int mb, int ntok) {
  BookAs book(m);
  const vdr_config& c = m->cfg;
  const int D = c.dim;
  // (fp8_cls_bf16: the CLS rows' MLP on the bf16 weights -- the explicit path)
  const BlockSteps b{m, s, w, L, c.fp8 && c.fp8_cls_bf16 && c.has_cls ? PATH_EXPLICIT : block_path(m)};
  // resid_fp32: the CLS rows' fp32 residual comes from x32 (strided) and stays in xc32 (compact)
  const Rows x{w.x, w.x32, ntok}, xc{w.h, w.x32 ? w.xc32 : nullptr, 0};
  // norm2 of the compact rows goes behind them in w.h (it holds Mp >= mb * ntok + 256 rows); as MX-fp8 its scales go to
  // w.hs (the layouts depend only on the row count each launch is given)
  char* hn = w.h + (size_t)round_up(mb, 256) * D * 2;
  LnFold prod;  // (the tail's producer always finalises the statistics of its rows)
  prod.part = w.part;
  prod.part_stride = w.Mp;
  prod.fin_stats = w.stats;
  int rc;
  if ((rc = b.resid_linear(false, mb, w.o, (int64_t)ntok * D, x, xc, b.path == PATH_FOLD ? &prod : nullptr))) return rc;
  if ((rc = b.norm_linear(true, mb, xc, hn, w.u, 0))) return rc;
  return b.resid_linear(true, mb, w.u, 0, xc, xc, nullptr);
}

// vdr_forward_layers: the outputs to write after each block, and the first image of the micro-batch being run
struct EmitList {
  std::vector<std::vector<const vdr_layer_out*>> at;  // [block] -> outputs of that block
  std::vector<std::vector<const vdr_attn_map*>> maps; // [block] -> attention maps of that block (vdr_forward_attn_maps)
  std::vector<std::vector<const vdr_facet_out*>> facets;  // [block] -> facets of that block (vdr_forward_facets)
  int last = -1;                                      // last block that runs (the largest requested layer)
  int b0 = 0;
};

// Writes one attention map for images b0 .. b0 + mb - 1 from the qkv activation of their micro-batch, right after the
// block's attention (nothing rewrites w.qkv before the next block's qkv GEMM, later on the same stream).  Booked as
// VDR_K_FINAL_LN, the class of every output write: three score products per map row, K read per pass.
int write_attn_map(vdr_model* m, hipStream_t s, const Carve& w, int mb, int ntok, const vdr_attn_map& a, int b0) {
  const vdr_config& c = m->cfg;
  const int H = c.heads, D = c.dim;
  const size_t es = a.out_dtype == VDR_BF16 ? 2 : 4;
  const size_t per_image = (size_t)(a.head_mean ? 1 : H) * a.q_rows * ntok;
  char* dst = (char*)a.out + (size_t)b0 * per_image * es;
  Scope sc(m, s, VDR_K_FINAL_LN, 6.0 * (double)mb * a.q_rows * ntok * D,
           (double)mb * (3.0 * ntok * D * 2 + (double)a.q_rows * D * 2 + (double)per_image * es));
  VDR_TRY(launch_attention_probs(w.qkv, dst, mb, ntok, H, D / H, a.q_rows, a.head_mean, a.out_dtype == VDR_BF16, s),
          "attention_probs");
  return VDR_OK;
}

// Writes one output for images b0 .. b0 + mb - 1 from the residual stream of their micro-batch, on its stream: the rows
// out_mode selects, through the model's final LayerNorm (norm = 1) or raw, read from the stream's fp32 master copy when
// there is one (resid_fp32), else from its bf16 rows.  vdr_forward and vdr_forward_tokens write their output after the
// last block (norm = pre_ln); vdr_forward_layers writes each of block i's right after the block's last residual GEMM (and,
// fp8_cls_bf16, after the copy that puts the CLS rows' bf16 MLP result into w.x: it is enqueued on `s` before this call,
// so stream order puts these reads behind it) -- the bits of a model truncated to i + 1 blocks.  compact: the block ran
// its CLS rows only (block_tail_cls) and they sit in w.h / w.xc32.  Every launch is booked as VDR_K_FINAL_LN.
int write_output(vdr_model* m, hipStream_t s, const Carve& w, int mb, int ntok, const vdr_layer_out& o, int b0, bool compact) {
  const vdr_config& c = m->cfg;
  // (ncls: the rows in front of the patch rows -- the CLS row and, on an image model, the register tokens, which DENSE
  // and POOLED discard with it)
  const int D = c.dim, ncls = c.patch ? prefix_rows(m) : (c.has_cls ? 1 : 0), n = ntok - ncls;
  const int ob = o.out_dtype == VDR_BF16;
  const size_t es = ob ? 2 : 4;
  const bool f32 = compact ? w.xc32 != nullptr : w.x32 != nullptr;
  const void* src = compact ? (f32 ? (const void*)w.xc32 : (const void*)w.h) : (f32 ? (const void*)w.x32 : (const void*)w.x);
  if (o.out_mode == VDR_OUT_POOLED) {
    const int64_t ld = o.ld ? o.ld : D;
    char* dst = (char*)o.out + (size_t)b0 * ld * es;
    if (pool_part_bytes(mb, n, D) > (size_t)w.Mp * c.mlp_hidden * 2)
      return fail(m, VDR_ERR_UNSUPPORTED, "pooled output: partial sums do not fit the MLP activation buffer");
    Scope sc(m, s, VDR_K_FINAL_LN, 0.0, (double)mb * n * D * (f32 ? 4 : 2) + (double)mb * D * es);
    // (the partial sums go to the fc1 activation w.u: dead from fc2 of block i to fc1 of block i + 1)
    VDR_TRY(launch_pool_rows(src, !f32, o.norm, m->normw, m->normb, c.ln_eps, mb, ntok, ncls, n, D, (float*)w.u, dst, ob, ld, s),
            "pooled rows");
    return VDR_OK;
  }
  RowMap im = identity_map();
  int64_t rows = mb, ld = 0;
  char* dst;
  if (o.out_mode == VDR_OUT_CLS) {
    if (!compact) im = RowMap{1, ntok, 0};
    ld = o.ld ? o.ld : D;
    dst = (char*)o.out + (size_t)b0 * ld * es;
  } else if (o.out_mode == VDR_OUT_DENSE) {
    im = RowMap{n, ntok, ncls};
    rows = (int64_t)mb * n;
    dst = (char*)o.out + (size_t)b0 * n * D * es;
  } else {
    rows = (int64_t)mb * ntok;
    dst = (char*)o.out + (size_t)b0 * ntok * D * es;
  }
  if (o.norm) return layernorm(m, s, VDR_K_FINAL_LN, src, !f32, dst, ob, m->normw, m->normb, rows, im, nullptr, 0, 0, ld);
  Scope sc(m, s, VDR_K_FINAL_LN, 0.0, (double)rows * D * ((f32 ? 4 : 2) + es));
  VDR_TRY(launch_gather_rows(src, dst, ob, rows, D, im, s, f32, ld), "gather_rows");
  return VDR_OK;
}

// Writes one facet (vdr_forward_facets) for images b0 .. b0 + mb - 1.  q / k / v: from the qkv activation of their
// micro-batch, right after the block's qkv GEMM (before the RoPE rotation and the attention); TOKEN: from the residual
// stream after the block, where write_output runs -- unbinned THROUGH write_output (the bits of a norm = 0 layer output).
// Binned: the log-bin kernel reads the patch rows where they lie; its level means go to the fc1 activation w.u, dead from
// fc2 of block i - 1 to fc1 of block i and from fc2 of block i on (as the pooled output's partial sums).  Booked as
// VDR_K_FINAL_LN.
int write_facet(vdr_model* m, hipStream_t s, const Carve& w, int mb, int ntok, const vdr_facet_out& f, int b0) {
  const vdr_config& c = m->cfg;
  const int D = c.dim, P = prefix_rows(m), n = ntok - P, h = f.hierarchy;
  const int ob = f.out_dtype == VDR_BF16;
  const size_t es = ob ? 2 : 4;
  const bool token = f.facet == VDR_FACET_TOKEN;
  if (token && !h) {
    vdr_layer_out o{};
    o.layer = f.layer;
    o.out_mode = f.all_rows ? VDR_OUT_TOKENS : VDR_OUT_DENSE;
    o.out_dtype = f.out_dtype;
    o.out = f.out;
    return write_output(m, s, w, mb, ntok, o, b0, false);
  }
  // the source rows: the stream (its fp32 master copy under resid_fp32), or the facet's columns of the qkv activation
  const bool f32 = token && w.x32 != nullptr;
  const int64_t ld = token ? D : 3 * D;
  const size_t ies = f32 ? 4 : 2;
  const char* src = token ? (f32 ? (const char*)w.x32 : (const char*)w.x) : (const char*)w.qkv + (size_t)(f.facet - VDR_FACET_QUERY) * D * 2;
  if (!h) {
    const int64_t rpi = f.all_rows ? ntok : n;
    char* dst = (char*)f.out + (size_t)b0 * rpi * D * es;
    Scope sc(m, s, VDR_K_FINAL_LN, 0.0, (double)mb * rpi * D * (2 + es));
    VDR_TRY(launch_gather_rows(src, dst, ob, (int64_t)mb * rpi, D, f.all_rows ? identity_map() : RowMap{n, ntok, P}, s, 0, 0, ld),
            "gather_rows(facet)");
    return VDR_OK;
  }
  // (forward_layers_impl has checked that the level means fit w.u and that D % 8 == 0)
  const int bins = 1 + 8 * h;
  char* dst = (char*)f.out + (size_t)b0 * n * bins * D * es;
  Scope sc(m, s, VDR_K_FINAL_LN, 0.0, (double)mb * n * D * (ies + (double)bins * es));
  VDR_TRY(launch_log_bin(src + (size_t)P * ld * ies, !f32, ld, (int64_t)ntok * ld, mb, grid_h(m), grid_w(m), D, h, (float*)w.u, dst, ob, s),
          "log_bin");
  return VDR_OK;
}

// What a forward asks of run_blocks beyond the rows themselves
struct BlockRun {
  const int* lens = nullptr;   // variable-length token sequences: the valid keys of each (device pointer), plus len_add
  int len_add = 0;
  bool cls_tail = false;       // the caller only wants the CLS rows of the last block (see block_tail_cls)
  const EmitList* el = nullptr;  // vdr_forward_layers: blocks 0 .. el->last run, each block's requested outputs are written after it
  bool compact = false;        // out: the last block ran its CLS rows only and left them in w.h [mb, D]
};

// L transformer blocks over x [M = mb*ntok rows]; leaves the result in w.x (r.compact: the CLS rows of it in w.h)
int run_blocks(vdr_model* m, hipStream_t s, const Carve& w, int mb, int ntok, BlockRun& r) {
  const vdr_config& c = m->cfg;
  const int D = c.dim, F = c.mlp_hidden, H = c.heads;
  const int64_t M = (int64_t)mb * ntok;
  const int N1 = fc1_epilogue(c) == EPI_SWIGLU ? 2 * F : F;
  const EmitList* el = r.el;
  int rc;
  r.compact = false;
  // (post-LN blocks keep every row: their last operation is a LayerNorm over the block's own output, also row-wise, but
  // the classifier that uses them is not a throughput path)
  const int nl = el ? el->last + 1 : c.layers;
  const int tail_at = (r.cls_tail && c.pre_ln && !c.full_last_block && ntok > 1) ? nl - 1 : -1;
  // (a block's outputs; the tail's CLS rows are compact)
  auto after = [&](int i, bool cmp) {
    if (el)
      for (const vdr_layer_out* o : el->at[i])
        if (int e = write_output(m, s, w, mb, ntok, *o, el->b0, cmp)) return e;
    // (TOKEN facets: a block that has one runs every row -- forward_layers_impl keeps the CLS tail off it)
    if (el && !cmp)
      for (const vdr_facet_out* f : el->facets[i])
        if (f->facet == VDR_FACET_TOKEN)
          if (int e = write_facet(m, s, w, mb, ntok, *f, el->b0)) return e;
    return (int)VDR_OK;
  };
  // vdr_forward_facets: block i's q / k / v facets, from its qkv, right after the qkv GEMM (before rope and attention)
  auto facets_after_qkv = [&](int i) {
    if (el)
      for (const vdr_facet_out* f : el->facets[i])
        if (f->facet != VDR_FACET_TOKEN)
          if (int e = write_facet(m, s, w, mb, ntok, *f, el->b0)) return e;
    return (int)VDR_OK;
  };
  auto has_token_facet = [&](int i) {
    for (const vdr_facet_out* f : el->facets[i])
      if (f->facet == VDR_FACET_TOKEN) return true;
    return false;
  };
  auto attention = [&]() {
    if (m->rope) {
      // DINOv3: q and k of the patch rows rotated in place between the qkv GEMM and everything that reads them (the
      // attention and, from the same buffer, the attention maps); booked with the token assembly
      const int P = prefix_rows(m);
      const double el = (double)mb * (ntok - P) * 2 * D;  // q and k elements
      Scope sc(m, s, VDR_K_ASSEMBLE, 3.0 * el, 4.0 * el);
      VDR_TRY(launch_rope2d(w.qkv, mb, ntok, P, H, D / H, m->rope_cos.as<float>(), m->rope_sin.as<float>(), s), "rope2d");
    }
    Scope sc(m, s, VDR_K_ATTENTION, 4.0 * (double)ntok * ntok * D * mb, 2.0 * (double)M * 4 * D);
    VDR_KNOB int attn_variant = env_int("VDR_ATTN_VARIANT", 0);  // (tuning builds)
    VDR_TRY(launch_attention(w.qkv, w.o, mb, ntok, H, attn_variant, s, nullptr, r.lens, r.len_add, D / H), "attention");
    return (int)VDR_OK;
  };
  // vdr_forward_attn_maps: block i's maps, from its qkv, right after its attention
  auto maps_after_attention = [&](int i) {
    if (el)
      for (const vdr_attn_map* a : el->maps[i])
        if (int e = write_attn_map(m, s, w, mb, ntok, *a, el->b0)) return e;
    return (int)VDR_OK;
  };
  // a last block whose only requests are maps stops after its attention
  auto maps_only_last = [&](int i) { return el && i == el->last && el->at[i].empty() && !has_token_facet(i); };
  const BlockPath path = block_path(m);
  // The fold's producers (proj, fc2) leave the partials and finalise the statistics where a consumer reads finalised ones;
  // launches small enough for the ring3 / ring4 consumers to finalise their own rows from the partials need nothing.
  LnFold fold_prod;
  if (path == PATH_FOLD) {
    fold_prod.part = w.part;
    fold_prod.part_stride = w.Mp;
    if (!ln_stats_in_gemm(VDR_K_GEMM_QKV, M, 3 * D, D / 64) || !ln_stats_in_gemm(VDR_K_GEMM_FC1, M, N1, D / 64))
      fold_prod.fin_stats = w.stats;
  }
  const LnFold* prod = path == PATH_FOLD ? &fold_prod : nullptr;
  // the stream, in place (with its fp32 master copy under resid_fp32); post-LN: the residual linears write w.h, the input
  // of the LayerNorm that follows each of them back into w.x
  const Rows x{w.x, w.x32, 0}, sum = c.pre_ln ? x : Rows{w.h, nullptr, 0};
  // vdr_config.fp8_cls_bf16 (image models with a CLS token; not the variable-length token path): the CLS rows' bf16 MLP
  // runs on the side stream ai under norm2 / fc1 of every row
  const int ai = m->cur_aux;
  const bool cls_bf16 = path == PATH_MX && c.fp8_cls_bf16 && c.has_cls && c.patch && ntok > 1 && !r.lens && ai < (int)m->aux.size() && w.cls_x;
  for (int i = 0; i < nl; ++i) {
    const LayerW& L = m->layers[i];
    const BlockSteps b{m, s, w, L, path};
    if ((rc = b.norm_linear(false, M, x, w.h, w.qkv, w.Mp))) return rc;
    if ((rc = facets_after_qkv(i))) return rc;
    // a last block whose only requests are q / k / v facets stops after its qkv GEMM
    if (maps_only_last(i) && el->maps[i].empty()) return VDR_OK;
    if ((rc = attention())) return rc;
    if ((rc = maps_after_attention(i))) return rc;
    if (maps_only_last(i)) return VDR_OK;
    if (i == tail_at) {  // the block ends after its attention: the rest of it on the CLS rows, then its outputs
      r.compact = true;
      if ((rc = block_tail_cls(m, s, w, L, mb, ntok))) return rc;
      return after(i, true);
    }
    if ((rc = b.resid_linear(false, M, w.o, 0, x, sum, prod))) return rc;
    if (!c.pre_ln && (rc = layernorm(m, s, VDR_K_LAYERNORM, w.h, 1, w.x, 1, L.n1w, L.n1b, M, identity_map()))) return rc;
    if (cls_bf16) {
      // fork: nothing writes w.x between here and fc2
      VDR_TRY(hipEventRecord(m->aux_fork[ai].get(), s), "hipEventRecord");
      VDR_TRY(hipStreamWaitEvent(m->aux[ai].get(), m->aux_fork[ai].get(), 0), "hipStreamWaitEvent");
      if ((rc = cls_mlp_bf16(m, m->aux[ai].get(), w, L, mb, ntok))) return rc;
      VDR_TRY(hipEventRecord(m->aux_join[ai].get(), m->aux[ai].get()), "hipEventRecord");
    }
    if ((rc = b.norm_linear(true, M, x, w.h, w.u, w.Mp))) return rc;
    // join: fc2 rewrites every row of w.x, the CLS rows' residual reads must be over
    if (cls_bf16) VDR_TRY(hipStreamWaitEvent(s, m->aux_join[ai].get(), 0), "hipStreamWaitEvent");
    if ((rc = b.resid_linear(true, M, w.u, 0, x, sum, prod))) return rc;
    if (!c.pre_ln && (rc = layernorm(m, s, VDR_K_LAYERNORM, w.h, 1, w.x, 1, L.n2w, L.n2b, M, identity_map()))) return rc;
    if (cls_bf16)  // ... and the bf16 result replaces the MX-fp8 one in the CLS rows
      VDR_TRY(hipMemcpy2DAsync(w.x, (size_t)ntok * D * 2, w.cls_x, (size_t)D * 2, (size_t)D * 2, (size_t)mb, hipMemcpyDeviceToDevice, s),
              "hipMemcpy2DAsync(CLS rows)");
    // (the outputs of block i read w.x after that copy: both are on s)
    if ((rc = after(i, false))) return rc;
  }
  return VDR_OK;
}

// SAM / MedSAM ImageEncoderViT blocks + neck over x [mb * g*g rows] (tokens NHWC, pos_embed already added).
// Window blocks: LN1 writes the window-partitioned, zero-padded order (padding rows of w.h stay zero),
// qkv / rel-pos / attention run on windows, the proj epilogue un-partitions while adding the residual.
// T[(token, head)][j] = q . table[j] for every relative offset j of both axes: one GEMM whose A rows are the
// per-head q slices of the packed qkv activation (M = tokens * heads, N = relpos_npad(S), K = 64), fp32 out.
hipError_t relpos_products(const void* qkv, const void* table, float* T, int64_t tokens, int S, int heads, hipStream_t s) {
  GemmArgs ga = linear(qkv, table, T, tokens * heads, relpos_npad(S), 64, EPI_BIAS);
  ga.a_rpg = heads;
  ga.a_gs = (int64_t)3 * heads * 64;
  ga.a_is = 64;
  ga.out_f32 = 1;
  // ring3 (the two-stride A gather): 128x128 tiles for the 64-column window table, 128x256 for the global one
  return launch_gemm(ga, EPI_BIAS, ga.N <= 128 ? VARIANT_RING3_128x128 : VARIANT_RING3_128x256, s);
}

// ---- the window steps of a SAM block, built in one place for run_sam and for the vdr_op_*_window entry points ----------
// `batch` grids of g x g tokens in ws x ws windows, nw = ceil(g / ws) a side, the border windows padded: rows of the
// window-partition order per grid (ws = 0, a global block: the grid itself)
int64_t sam_window_rows(int g, int ws) {
  if (ws <= 0) return (int64_t)g * g;
  const int64_t nw = (g + ws - 1) / ws;
  return nw * nw * ws * ws;
}

// norm1: tokens x [batch * g * g, D] bf16 -> y bf16, in window-partition order (padding rows are not written) or, ws = 0, as they are
LnArgs sam_ln_args(const void* x, void* y, const float* gw, const float* gb, float eps, int batch, int g, int ws, int D) {
  LnArgs a{};
  a.x = x;
  a.in_bf16 = 1;
  a.y = y;
  a.out_bf16 = 1;
  a.gamma = gw;
  a.beta = gb;
  a.rows = (int64_t)batch * g * g;
  a.D = D;
  a.eps = eps;
  a.imap = identity_map();
  a.omap = identity_map();
  a.win_ws = ws;
  a.win_g = ws ? g : 0;
  return a;
}

// the same with MX-fp8 output: the scale array is that of a tensor of batch * sam_window_rows(g, ws) rows
hipError_t sam_ln_mx(const void* x, const float* gw, const float* gb, float eps, int batch, int g, int ws, int D, void* q,
                     void* scales, hipStream_t s) {
  return launch_ln_mx(x, gw, gb, eps, (int64_t)batch * g * g, D, q, scales, s, ws, g, batch * sam_window_rows(g, ws));
}

// the out-projection: y[unpart(r)] = resid[unpart(r)] + a[r] . W^T + bias over the batch * sam_window_rows(g, ws) rows of a
// (padding rows dropped; ws = 0: unpart is the identity), y may be resid; part non-null: the LayerNorm partials of y's rows
GemmArgs sam_proj_args(const void* a, const void* W, const float* bias, const void* resid, void* y, int batch, int g, int ws,
                       int N, int K, float* part, int64_t part_stride) {
  GemmArgs ga = linear(a, W, y, batch * sam_window_rows(g, ws), N, K, EPI_BIAS_RESID);
  ga.bias = bias;
  ga.resid = resid;
  if (ws) {
    ga.win_ws = ws;
    ga.win_g = g;
  }
  if (part) {
    ga.ln_part = part;
    ga.part_stride = part_stride;
  }
  return ga;
}

int run_sam(vdr_model* m, hipStream_t s, const Carve& w, int mb, int out_dtype, char* out, bool tokens_only) {
  const vdr_config& c = m->cfg;
  const int D = c.dim, H = c.heads, C = c.neck_chans;
  const int g = c.img / c.patch, n = g * g, ws = c.window, nw = (g + ws - 1) / ws, wtok = nw * nw * ws * ws;
  const int64_t M = (int64_t)mb * n;
  int rc;
  VDR_TRY(hipMemsetAsync(w.h, 0, (size_t)mb * wtok * D * 2, s), "memset(window padding)");
  // fp8 (qkv / fc1 / fc2 on the block-scaled MFMA; out-projection, rel-pos GEMM, attention and neck stay bf16): the
  // padding rows of the windowed MX activation are zero payload (memset above) under zeroed, i.e. finite, scales
  const bool fp8 = c.fp8 != 0;
  if (fp8) VDR_TRY(hipMemsetAsync(w.hs, 0, mx_scale_bytes(w.Mp, D), s), "memset(window padding scales)");
  const BlockPath path = block_path(m);
  const Rows x{w.x, w.x32, 0};
  for (int i = 0; i < c.layers; ++i) {
    const LayerW& L = m->layers[i];
    const bool glob = (c.global_mask >> i) & 1;
    const int S = glob ? g : ws;
    const int64_t T = glob ? M : (int64_t)mb * wtok;
    const int nb = glob ? mb : mb * nw * nw;
    char* hbuf = glob ? w.hg : w.h;
    if (fp8) {
      {
        Scope sc(m, s, VDR_K_LAYERNORM, 0.0, (double)M * D * 3);
        VDR_TRY(sam_ln_mx(w.x, L.n1w, L.n1b, c.ln_eps, mb, g, glob ? 0 : ws, D, hbuf, w.hs, s), "layernorm_mx(window)");
      }
      if ((rc = gemm_mx(m, s, VDR_K_GEMM_QKV, hbuf, w.hs, L.qkv_q.get(), L.qkv_s.get(), L.bqkv, nullptr, nullptr, w.qkv, nullptr, T, 3 * D, D, EPI_BIAS)))
        return rc;
    } else {
      if ((rc = layernorm(m, s, VDR_K_LAYERNORM, sam_ln_args(w.x, hbuf, L.n1w, L.n1b, c.ln_eps, mb, g, glob ? 0 : ws, D)))) return rc;
      GemmArgs qkv = linear(hbuf, L.wqkv, w.qkv, T, 3 * D, D, EPI_BIAS);
      qkv.bias = L.bqkv;
      qkv.a_rows = w.Mp;
      if ((rc = gemm(m, s, VDR_K_GEMM_QKV, qkv, EPI_BIAS))) return rc;
    }
    {
      Scope sc(m, s, VDR_K_ATTENTION, 4.0 * (double)S * S * S * S * 64.0 * H * nb + 2.0 * T * H * relpos_npad(S) * 64,
               2.0 * (double)T * 4 * D);
      VDR_TRY(relpos_products(w.qkv, L.reltab.get(), w.rel, T, S, H, s), "relpos");
      VDR_TRY(launch_attention_relpos(w.qkv, w.rel, w.o, nb, S, H, s, glob ? env_int("VDR_RELPOS_ANY", 0) : 0), "attention_relpos");
    }
    {
      // (not through gemm(): the profiler books T rows of A, the windowed ones with their padding, but M output rows)
      GemmArgs ga = sam_proj_args(w.o, L.wproj, L.bproj, w.x, w.x, mb, g, glob ? 0 : ws, D, D, m->ln_fuse ? w.part : nullptr, w.Mp);
      Scope sc(m, s, VDR_K_GEMM_PROJ, 2.0 * T * D * D, 2.0 * ((double)T * D + (double)D * D + 2.0 * M * D));
      VDR_TRY(launch_gemm_w(m, ga, EPI_BIAS_RESID, gemm_variant_for(VDR_K_GEMM_PROJ, ga.M, ga.N), s), "proj gemm");
      m->stats_fresh = false;  // (window un-partition scatters the rows: their statistics are finalised by ln_consumer's launch)
    }
    // the MLP half is the plain block's (GELU, no LayerScale); fc2 produces no partials: the next block's qkv is not folded
    const BlockSteps b{m, s, w, L, path};
    if ((rc = b.norm_linear(true, M, x, w.hg, w.u, w.Mp))) return rc;
    if ((rc = b.resid_linear(true, M, w.u, 0, x, x, nullptr))) return rc;
  }
  if (tokens_only) {
    Scope sc(m, s, VDR_K_FINAL_LN, 0.0, (double)M * D * 6);
    VDR_TRY(launch_gather_rows(w.x, out, out_dtype == VDR_BF16, M, D, identity_map(), s), "gather_rows");
    return VDR_OK;
  }
  // neck: 1x1 conv (no bias) -> LayerNorm2d -> 3x3 conv pad 1 (no bias) -> LayerNorm2d, all on NHWC tokens
  if ((rc = gemm(m, s, VDR_K_GEMM_PATCH, linear(w.x, m->w_neck0, w.qkv, M, C, D, EPI_BIAS), EPI_BIAS))) return rc;
  if ((rc = layernorm(m, s, VDR_K_FINAL_LN, w.qkv, 1, w.o, 1, m->neck1w, m->neck1b, M, identity_map(), nullptr, 0, C))) return rc;
  {
    Scope sc(m, s, VDR_K_IM2COL, 0.0, (double)M * C * 2 * 10);
    VDR_TRY(launch_im2col3(w.o, w.u, mb, g, C, s), "im2col3");
  }
  if ((rc = gemm(m, s, VDR_K_GEMM_PATCH, linear(w.u, m->w_neck2, w.hg, M, C, 9 * C, EPI_BIAS), EPI_BIAS))) return rc;
  return layernorm(m, s, VDR_K_FINAL_LN, w.hg, 1, out, out_dtype == VDR_BF16, m->neck3w, m->neck3b, M, identity_map(), nullptr,
                   0, C);
}

// patch embedding of one micro-batch: the token rows b*ntok + P + i of w.x (P prefix rows; pos_embed added), or -- pe_out non-null,
// model.patch_embed(x) -- the caller's [mb, n, D] output
int embed_patches(vdr_model* m, hipStream_t s, const Carve& w, const char* img, int in_dtype, int mb, char* pe_out, int out_dtype) {
  const vdr_config& c = m->cfg;
  const int ntok = m->n_tokens, n = m->n_patches, D = c.dim, ncls = prefix_rows(m);
  const bool pe_only = pe_out != nullptr;
  GemmArgs g;
  int variant;
  VDR_TRY(patch_gemm(m, s, img, in_dtype, w.u, m->w_patch, pe_only ? (void*)pe_out : (void*)w.x, mb, c.in_chans, m->in_h, m->in_w, c.patch,
                     m->stride, D, &g, &variant),
          "im2col");
  g.bias = m->b_patch;
  if (pe_only) {
    // model.patch_embed(x) (tfds_dense_descriptor.py:128): the GEMM epilogue writes the caller's [B, n, D] buffer
    // directly, bf16 or fp32 (no conversion pass)
    g.out_f32 = out_dtype != VDR_BF16;
    g.omap = RowMap{n, n, 0};
  } else {
    g.pos = m->pos;
    g.omap = RowMap{n, ntok, ncls};
    if (m->ln_fuse && !c.input_ln) {  // (input_ln: the input LayerNorm leaves the statistics, those of the raw rows are not wanted)
      g.ln_part = w.part;
      g.part_stride = w.Mp;
    }
  }
  Scope sc(m, s, VDR_K_GEMM_PATCH, 2.0 * g.M * D * c.in_chans * c.patch * c.patch,
           2.0 * ((double)g.M * m->Kp + (double)D * m->Kp + (double)g.M * D));
  VDR_TRY(launch_gemm_w(m, g, EPI_PATCH, variant, s), "patch gemm");
  return VDR_OK;
}

// CLS / register rows, input LayerNorm and the fp32 master copy of the stream: afterwards w.x (w.x32) holds what block 0 reads
int assemble_stream(vdr_model* m, hipStream_t s, const Carve& w, int mb, int ntok) {
  const vdr_config& c = m->cfg;
  const int D = c.dim;
  int rc;
  if (c.has_cls) {
    Scope sc(m, s, VDR_K_ASSEMBLE, 0.0, (double)mb * (1 + m->n_reg) * D * 2);
    if (m->ln_fuse && !c.input_ln)
      VDR_TRY(launch_prefix_rows_stats(m->cls, m->pos, m->reg, m->n_reg, w.x, w.part, w.Mp, mb, ntok, D, s), "prefix rows");
    else
      VDR_TRY(launch_prefix_rows(m->cls, m->pos, m->reg, m->n_reg, w.x, mb, ntok, D, s), "prefix rows");
  }
  if (c.input_ln && m->ln_fuse) {
    // in place, and the (sum, sumsq) partials of the normalised rows -- block 0's folded qkv GEMM reads them where the
    // patch epilogue and the CLS rows leave those of the raw rows in a model without input_ln (here they leave none)
    Scope sc(m, s, VDR_K_LAYERNORM, 0.0, (double)mb * ntok * D * 4);
    VDR_TRY(launch_ln_rows_stats(w.x, m->inw, m->inb, c.ln_eps, (int64_t)mb * ntok, D, w.part, w.Mp, s), "input layernorm");
  } else if (c.input_ln) {
    if ((rc = layernorm(m, s, VDR_K_LAYERNORM, w.x, 1, w.x, 1, m->inw, m->inb, (int64_t)mb * ntok, identity_map())))
      return rc;
  }
  if (w.x32) {  // resid_fp32: the stream's fp32 master copy starts from the assembled tokens (their one bf16 rounding stays)
    Scope sc(m, s, VDR_K_ASSEMBLE, 0.0, (double)mb * ntok * D * 6);
    VDR_TRY(launch_gather_rows(w.x, w.x32, 0, (int64_t)mb * ntok, D, identity_map(), s), "residual stream -> fp32");
  }
  return VDR_OK;
}

int check_device(vdr_handle h) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    return fail(h, VDR_ERR_NO_DEVICE, "no HIP device visible: libvdr has no CPU path");
  }
  return VDR_OK;
}

// ---- micro-batches ------------------------------------------------------------------------------------------------------
// The 8-phase rounds of the block loop's qkv / fc1 launch over `images` images; 0 where gemm() gives the launch to another
// tile variant.  gemm()'s own test (takes_8p) on the launch as BlockSteps::norm_linear describes it: dense operands, the
// workspace rows readable past the last tile.
int64_t block_linear_rounds(const vdr_model* m, bool fc1, int images, int ntok, double* idle = nullptr) {
  const vdr_config& c = m->cfg;
  if (idle) *idle = 0.0;
  if (c.fp8) return 0;  // (PATH_MX: gemm_mx)
  const int epi = fc1 ? fc1_epilogue(c) : EPI_BIAS;
  const int N = !fc1 ? 3 * c.dim : epi == EPI_SWIGLU ? 2 * c.mlp_hidden : c.mlp_hidden;
  GemmArgs g = linear(nullptr, nullptr, nullptr, (int64_t)images * ntok, N, c.dim, epi);
  g.a_rows = (g.M + 255) / 256 * 256 + 256;  // (carve: Mp of a slice that holds at least these images)
  return takes_8p(fc1 ? VDR_K_GEMM_FC1 : VDR_K_GEMM_QKV, g, epi) ? gemm_8p_rounds(g.M, g.N, idle) : 0;
}

// The default split (vdr_config.micro_batch == 0 and streams == 0): two parts on two internal streams, so that the idle
// time between one part's launches -- per-launch intercepts, ln_finalize, the CLS tail: 6-7 % of the ViT-B batch-256 step --
// runs under the other part's kernels.  The 8-phase GEMMs run whole rounds of one workgroup per CU, so a split
// pays only where it adds no round: a candidate (b1, batch - b1) is admissible when every qkv / fc1 launch that takes tile
// variant 31 for the whole batch takes it for both parts and the parts' summed rounds do not exceed the whole batch's
// (ViT-B at 256: 7 + 10 whole, 18 for 128 + 128, 17 for 146 + 110).  Fewest summed rounds win, then the most even pair.
// The summed rounds never fall below the whole batch's, so what the second stream recovers inside these GEMMs is the part
// of a round that the whole batch's last rounds leave the chip empty; the split itself costs about 0.2 ms of a ViT-B step
// (the ramps of twice the launches), which is 3/4 of a round per block there: a batch whose qkv and fc1 launches leave less
// than SPLIT_MIN_IDLE of a round idle between them stays whole (ViT-B: 320, 384, 512; measured at 384: 12.87 -> 13.04 ms).
// Returns the larger, first part; 0: no admissible pair, the forward runs the whole batch on the caller's stream.  Left
// alone, for want of a measurement: batches no launch of which takes variant 31, fp8 models and SAM encoders.
constexpr double SPLIT_MIN_IDLE = 0.75;
int default_split(vdr_model* m, int batch, int ntok) {
  const vdr_config& c = m->cfg;
  if (c.fp8 || c.window > 0 || c.layers <= 0 || batch < 2) return 0;
  if (m->split_batch == batch && m->split_ntok == ntok) return m->split_first;
  double idle[2];
  const int64_t whole[2] = {block_linear_rounds(m, false, batch, ntok, &idle[0]), block_linear_rounds(m, true, batch, ntok, &idle[1])};
  int first = 0;
  int64_t best = whole[0] + whole[1] + 1;
  for (int b1 = (batch + 1) / 2; b1 < batch && idle[0] + idle[1] >= SPLIT_MIN_IDLE; ++b1) {
    int64_t sum = 0;
    bool kept = true;
    for (int fc1 = 0; fc1 < 2; ++fc1) {
      const int64_t r1 = block_linear_rounds(m, fc1, b1, ntok), r2 = block_linear_rounds(m, fc1, batch - b1, ntok);
      kept = kept && (!whole[fc1] || (r1 && r2));
      sum += r1 + r2;
    }
    if (kept && sum < best) {  // (b1 ascending: of equal sums the most even pair stays)
      best = sum;
      first = b1;
    }
  }
  m->split_batch = batch;
  m->split_ntok = ntok;
  m->split_first = first;
  return first;
}

// How a forward cuts its batch: `parts` micro-batches of mb images (the last one the rest), part k on internal stream
// k % streams (streams == 1: the caller's) in workspace slice k % streams, each of `slice` bytes and carved for mb images.
struct BatchPlan {
  int mb, parts, streams;
  bool by_default;  // default_split chose it (not vdr_config.micro_batch / streams)
  size_t slice;
  size_t bytes;     // the workspace of the call: what vdr_workspace_bytes reports and every forward asks for
};

// The one place that decides it, for vdr_workspace_bytes, the forwards and the workspace carve alike.  linear_only: the
// caller's stream is being captured -- the default split stays out, so that a captured forward is a linear graph; `bytes` is
// the same either way and covers both forms.
BatchPlan batch_plan(vdr_model* m, int batch, int ntok, bool linear_only = false) {
  const vdr_config& c = m->cfg;
  BatchPlan p{};
  p.streams = configured_streams(m);
  p.mb = c.micro_batch > 0 ? (c.micro_batch < batch ? c.micro_batch : batch) : (batch + p.streams - 1) / p.streams;
  const int first = c.micro_batch == 0 && c.streams == 0 ? default_split(m, batch, ntok) : 0;
  p.by_default = first > 0;
  if (first && !linear_only) {
    p.mb = first;
    p.streams = 2;
  }
  p.parts = (batch + p.mb - 1) / p.mb;
  p.slice = carve(m, nullptr, p.mb, ntok).total;
  p.bytes = p.slice * p.streams;
  if (first) {  // (two slices for the larger part, or the whole batch in one)
    const size_t two = 2 * carve(m, nullptr, first, ntok).total, whole = carve(m, nullptr, batch, ntok).total;
    p.bytes = two > whole ? two : whole;
  }
  return p;
}

bool being_captured(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess) {  // (the legacy stream while another thread captures: stay linear)
    (void)hipGetLastError();
    return true;
  }
  return st != hipStreamCaptureStatusNone;
}

// The rest of every forward once its arguments are checked: the device, the workspace, then the micro-batches of
// batch_plan, each in its stream's slice of the workspace.  body(s, w, b0, mb) enqueues the micro-batch of images
// b0 .. b0 + mb - 1.
template <class Body>
int run_micro_batches(vdr_model* m, int batch, int ntok, void* workspace, size_t workspace_bytes, void* stream, Body body) {
  int rc = check_device(m);
  if (rc) return rc;
  if (!m->resolved) return fail(m, VDR_ERR_INCOMPLETE, "vdr_finalize has not run since the last vdr_set_weight");
  DeviceGuard dg(m->device);
  if (!dg.ok) return fail(m, VDR_ERR_HIP, "hipSetDevice failed");
  hipStream_t caller = (hipStream_t)stream;
  BatchPlan p = batch_plan(m, batch, ntok);
  if (p.bytes > workspace_bytes)
    return fail(m, VDR_ERR_WORKSPACE, "workspace too small: need " + std::to_string(p.bytes) + " bytes");
  if (p.by_default && being_captured(caller)) p = batch_plan(m, batch, ntok, true);
  const int ns = p.streams;
  if (fork_streams(m, caller, ns)) return fail(m, VDR_ERR_HIP, "internal stream setup failed");
  int chunk = 0;
  for (int b0 = 0; b0 < batch; b0 += p.mb, ++chunk) {
    const int mb = batch - b0 < p.mb ? batch - b0 : p.mb;
    const int si = chunk % ns;
    m->cur_aux = si;
    m->stats_fresh = false;  // (nothing has finalised the statistics of this micro-batch yet)
    hipStream_t s = ns == 1 ? caller : m->streams[si].get();
    const Carve w = carve(m, (char*)workspace + si * p.slice, p.mb, ntok);
    if ((rc = body(s, w, b0, mb))) return rc;
  }
  if (join_streams(m, caller, ns)) return fail(m, VDR_ERR_HIP, "internal stream join failed");
  return VDR_OK;
}

}  // namespace

// =================================================================================================
extern "C" {

int vdr_abi_version(void) { return VDR_ABI_VERSION; }

int vdr_tuning_build(void) {
#ifdef VDR_TUNING
  return 1;
#else
  return 0;
#endif
}

int vdr_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

const char* vdr_last_error(vdr_handle h) { return h ? h->err.c_str() : g_err.c_str(); }

const char* vdr_kernel_class_name(int k) {
  static const char* names[VDR_K_COUNT] = {"im2col",   "gemm_patch", "layernorm", "gemm_qkv", "attention", "gemm_proj",
                                           "gemm_fc1", "gemm_fc2",   "final_ln",  "assemble", "cls_tail"};
  return (k >= 0 && k < VDR_K_COUNT) ? names[k] : "?";
}

int vdr_create(const vdr_config* cfg, int device, vdr_handle* out) { return vdr_create_ext(cfg, nullptr, device, out); }

int vdr_create_ext(const vdr_config* cfg, const vdr_config_ext* ext, int device, vdr_handle* out) {
  if (!cfg || !out) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  const vdr_config& c = *cfg;
  vdr_config_ext x{};  // (null ext: no register tokens, no RoPE -- vdr_create)
  x.size = (int32_t)sizeof(vdr_config_ext);
  x.rope_theta = 100.0f;
  if (ext) {
    if (ext->size < (int32_t)sizeof(vdr_config_ext))
      return fail(nullptr, VDR_ERR_INVALID, "vdr_config_ext: size " + std::to_string(ext->size) + " is smaller than the " +
                                                std::to_string(sizeof(vdr_config_ext)) + " bytes of the fields this library knows");
    x = *ext;
  }
  if (c.dim <= 0 || c.heads <= 0 || c.layers < 0 || c.mlp_hidden <= 0)
    return fail(nullptr, VDR_ERR_INVALID, "dim/heads/layers/mlp_hidden must be positive");
  {
    const int dh = c.dim / c.heads;
    if (c.dim % c.heads || !head_dim_ok(dh))
      return fail(nullptr, VDR_ERR_UNSUPPORTED, "head dim must be 32, 64, 96 or 128 (dim == head dim * heads)");
    // the MX-fp8 attention output and its scales are laid out per 64 channels; the SAM rel-pos tables are [2S-1, 64]
    if (dh != 64 && c.fp8) return fail(nullptr, VDR_ERR_UNSUPPORTED, "fp8 = 1 needs head dim 64");
    if (dh != 64 && c.window > 0) return fail(nullptr, VDR_ERR_UNSUPPORTED, "windowed (SAM) attention needs head dim 64");
  }
  if (c.dim % 64 || c.mlp_hidden % 64 || c.dim > 2048)
    return fail(nullptr, VDR_ERR_UNSUPPORTED, "dim and mlp_hidden must be multiples of 64, dim <= 2048");
  if (c.patch) {
    if (c.img <= 0 || c.img % c.patch || c.in_chans <= 0) return fail(nullptr, VDR_ERR_INVALID, "img must be a multiple of patch");
  } else if (c.has_pos) {
    return fail(nullptr, VDR_ERR_UNSUPPORTED, "token models carry no learned pos_embed");
  }
  if (c.act < VDR_ACT_GELU || c.act > VDR_ACT_GELU_TANH) return fail(nullptr, VDR_ERR_INVALID, "unknown activation");
  if (c.fp8 == 1 && (c.act == VDR_ACT_QUICK_GELU || c.act == VDR_ACT_GELU_TANH))
    return fail(nullptr, VDR_ERR_UNSUPPORTED, "fp8 = 1: the MX-fp8 GEMM carries erf-GELU and SwiGLU only (QuickGELU / tanh-GELU: bf16 path)");
  if (c.fp8 && !c.pre_ln) return fail(nullptr, VDR_ERR_UNSUPPORTED, "fp8 weights: pre-LN models only");
  if (c.fp8_cls_bf16 < 0 || c.fp8_cls_bf16 > 1) return fail(nullptr, VDR_ERR_INVALID, "fp8_cls_bf16 must be 0 or 1");
  if (c.resid_fp32 < 0 || c.resid_fp32 > 1) return fail(nullptr, VDR_ERR_INVALID, "resid_fp32 must be 0 or 1");
  if (c.fp8 < 0 || c.fp8 > 1)
    return fail(nullptr, VDR_ERR_UNSUPPORTED,
                "fp8 must be 0 or 1 (a level that also quantised the out-projection measured 0.987 row cosine at 40 "
                "blocks, below the 0.99 gate, and is not shipped)");
  if (x.n_register < 0) return fail(nullptr, VDR_ERR_INVALID, "n_register must be >= 0");
  if (x.rope != 0 && x.rope != 1) return fail(nullptr, VDR_ERR_INVALID, "rope must be 0 or 1");
  if (x.n_register > 0 && !c.has_cls) return fail(nullptr, VDR_ERR_INVALID, "n_register > 0 needs has_cls = 1 (registers sit behind the CLS row)");
  if (x.rope && !(std::isfinite(x.rope_theta) && x.rope_theta > 1.0f))
    return fail(nullptr, VDR_ERR_INVALID, "rope = 1: rope_theta must be finite and > 1 (DINOv3: 100)");
  if (x.n_register > 0 || x.rope) {
    const char* what = x.rope ? "rope = 1" : "n_register > 0";
    if (x.n_register > 16) return fail(nullptr, VDR_ERR_UNSUPPORTED, "n_register must be at most 16");
    if (c.fp8) return fail(nullptr, VDR_ERR_UNSUPPORTED, std::string(what) + ": bf16 path only (fp8 = 1 is not covered)");
    if (c.window > 0) return fail(nullptr, VDR_ERR_UNSUPPORTED, std::string(what) + ": not for the SAM encoder (window > 0)");
    if (!c.patch) return fail(nullptr, VDR_ERR_UNSUPPORTED, std::string(what) + ": image models only (patch == 0 is a token model)");
    if (!c.pre_ln) return fail(nullptr, VDR_ERR_UNSUPPORTED, std::string(what) + ": pre-LN models only");
    if (x.rope && c.has_pos)
      return fail(nullptr, VDR_ERR_UNSUPPORTED, "rope = 1 with has_pos = 1: a RoPE model carries no learned pos_embed");
    if (x.rope && c.dim / c.heads == 96)
      return fail(nullptr, VDR_ERR_UNSUPPORTED, "rope = 1: head dim 32, 64 or 128 (96: its frequency step is inexact in fp32 and no checkpoint uses it)");
  }
  if (c.window > 0) {
    const int g = c.patch ? c.img / c.patch : 0;
    auto side_ok = [](int v) { return v == 4 || v == 7 || v == 10 || v == 14; };
    if (!c.patch || c.has_cls || !c.has_pos || !c.pre_ln || c.input_ln || c.layerscale || c.act != VDR_ACT_GELU)
      return fail(nullptr, VDR_ERR_INVALID, "SAM encoder: needs patch > 0, has_cls = 0, has_pos = 1, pre_ln = 1, GELU, no LayerScale");
    if (c.neck_chans <= 0 || c.neck_chans % 64 || c.neck_chans > 2048)
      return fail(nullptr, VDR_ERR_UNSUPPORTED, "SAM encoder: neck_chans must be a positive multiple of 64");
    if (!side_ok(c.window)) return fail(nullptr, VDR_ERR_UNSUPPORTED, "SAM encoder: window side in {4,7,10,14}");
    if (c.global_mask && g > 64)
      return fail(nullptr, VDR_ERR_UNSUPPORTED,
                  "SAM encoder: the grid side of global blocks (img / patch = " + std::to_string(g) +
                      ") must be at most 64: the packed rel-pos operand holds 127 + 127 rows");
    if (c.layers > 31) return fail(nullptr, VDR_ERR_UNSUPPORTED, "SAM encoder: at most 31 blocks");
  }
  int rc = check_device(nullptr);
  if (rc) return rc;
  int ndev = 0;
  hipGetDeviceCount(&ndev);
  if (device < 0 || device >= ndev) return fail(nullptr, VDR_ERR_INVALID, "device index out of range");
  std::unique_ptr<vdr_model> m(new vdr_model());
  m->cfg = c;
  m->device = device;
  m->n_reg = x.n_register;
  m->rope = x.rope;
  m->rope_theta = x.rope_theta;
  if (c.patch) {
    set_geometry(m.get(), c.img, c.img, c.patch);
    m->Kp = round_up(c.in_chans * c.patch * c.patch, 64);
  }
  m->layers.resize(c.layers);  // (before build_slots: the slots point into it)
  build_slots(m.get());
  *out = m.release();
  return VDR_OK;
}

void vdr_destroy(vdr_handle h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  delete h;  // (every device buffer, stream and event is a member that frees itself)
}

int vdr_num_weights(vdr_handle h) { return h ? (int)h->slots.size() : 0; }

const char* vdr_weight_name(vdr_handle h, int i) {
  if (!h || i < 0 || i >= (int)h->slots.size()) return nullptr;
  return h->slots[i].name.c_str();
}

int vdr_set_weight(vdr_handle m, const char* name, const float* host, const int64_t* shape, int ndim) {
  if (!m || !name || !host || (ndim > 0 && !shape)) return fail(m, VDR_ERR_INVALID, "null argument");
  auto it = m->index.find(name);
  if (it == m->index.end()) return fail(m, VDR_ERR_UNKNOWN_NAME, std::string("unknown weight name: ") + name);
  WSlot& s = m->slots[it->second];
  int64_t numel = 1;
  for (int i = 0; i < ndim; ++i) numel *= shape[i];
  // SAM handle, a table at another (native) grid than the handle's: pos_embed [1, g0, g0, D], rel_pos_h / rel_pos_w of a
  // global block [2 g0 - 1, 64], g0 in 1..64
  int64_t src_n = 0;
  if (numel != s.numel && s.resample == RS_POS && ndim == 4 && shape[0] == 1 && shape[1] == shape[2] && shape[1] >= 1 &&
      shape[1] <= 64 && shape[3] == m->cfg.dim)
    src_n = shape[1];
  if (numel != s.numel && s.resample == RS_REL && ndim == 2 && shape[1] == 64 && shape[0] >= 1 && shape[0] <= 127 &&
      (shape[0] & 1))
    src_n = shape[0];
  if (numel != s.numel && !src_n)
    return fail(m, VDR_ERR_INVALID, std::string(name) + ": expected " + std::to_string(s.numel) + " elements, got " +
                                        std::to_string(numel));
  DeviceGuard dg(m->device);
  if (!dg.ok) return fail(m, VDR_ERR_HIP, "hipSetDevice failed");
  if (src_n) {  // kept as loaded; vdr_finalize resamples it
    if (int rc = reserve(m, s.dev_src, (size_t)numel * 4, REPLACE, "native table")) return rc;
    VDR_TRY(hipMemcpy(s.dev_src.get(), host, (size_t)numel * 4, hipMemcpyHostToDevice), "hipMemcpy(native table)");
    s.host.assign(host, host + numel);
    s.src_n = src_n;
    s.set = true;
    m->resolved = false;
    return VDR_OK;
  }
  s.src_n = 0;
  std::vector<uint16_t> bf;
  std::vector<float> fv;
  const void* src = host;
  size_t bytes = 0;
  const int F = m->cfg.mlp_hidden;
  switch (s.kind) {
    case W_VEC_F32:
      bytes = (size_t)numel * 4;
      break;
    case W_MAT_BF16:
      bf.resize(numel);
      for (int64_t i = 0; i < numel; ++i) bf[i] = f32_to_bf16(host[i]);
      src = bf.data();
      bytes = (size_t)numel * 2;
      break;
    case W_PATCH_BF16: {
      // [D, C*p*p] -> [D, Kp] zero padded along k
      const int64_t K = s.cols, Kp = m->Kp;
      bf.assign((size_t)s.rows * Kp, 0);
      for (int64_t r = 0; r < s.rows; ++r)
        for (int64_t k = 0; k < K; ++k) bf[r * Kp + k] = f32_to_bf16(host[r * K + k]);
      src = bf.data();
      bytes = bf.size() * 2;
      break;
    }
    case W_W12_BF16: {
      // SwiGLU: interleave x1/x2 rows in blocks of 32 so one wave tile holds a gate pair (swiglu_source_row)
      if (F % 32) return fail(m, VDR_ERR_UNSUPPORTED, "SwiGLU hidden must be a multiple of 32");
      const int64_t K = s.cols;
      bf.resize(numel);
      for (int64_t pr = 0; pr < 2 * F; ++pr) {
        const int64_t srow = swiglu_source_row(pr, F);
        for (int64_t k = 0; k < K; ++k) bf[pr * K + k] = f32_to_bf16(host[srow * K + k]);
      }
      src = bf.data();
      bytes = (size_t)numel * 2;
      break;
    }
    case W_CONV3_BF16: {
      // [C_out, C_in, 3, 3] -> [C_out][j * C_in + c], j = ky*3 + kx (tap-major so that im2col3 moves
      // 8 channels of one tap with a single 16-byte load)
      const int64_t Cin = s.cols / 9;
      bf.resize(numel);
      for (int64_t co = 0; co < s.rows; ++co)
        for (int64_t ci = 0; ci < Cin; ++ci)
          for (int64_t j = 0; j < 9; ++j) bf[co * s.cols + j * Cin + ci] = f32_to_bf16(host[(co * Cin + ci) * 9 + j]);
      src = bf.data();
      bytes = (size_t)numel * 2;
      break;
    }
    case W_W12_BIAS: {
      fv.resize(numel);
      for (int64_t pr = 0; pr < 2 * F; ++pr) fv[pr] = host[swiglu_source_row(pr, F)];
      src = fv.data();
      bytes = (size_t)numel * 4;
      break;
    }
  }
  s.host.assign(host, host + numel);
  if (int rc = reserve(m, s.dev, bytes, IF_EMPTY, "weight")) return rc;
  VDR_TRY(hipMemcpy(s.dev.get(), src, bytes, hipMemcpyHostToDevice), "hipMemcpy(weight)");
  s.set = true;
  m->resolved = false;
  return VDR_OK;
}

int vdr_finalize(vdr_handle m) {
  if (!m) return fail(m, VDR_ERR_INVALID, "null handle");
  int rc = check_device(m);
  if (rc) return rc;
  DeviceGuard dg(m->device);
  if (!dg.ok) return fail(m, VDR_ERR_HIP, "hipSetDevice failed");
  if (m->resolved) return VDR_OK;
  return resolve(m);
}

int vdr_set_input_size(vdr_handle m, int height, int width) {
  // the argument checks that need no handle come first (they also hold for a null one)
  if (height <= 0) return fail(m, VDR_ERR_INVALID, "vdr_set_input_size: height must be positive");
  if (width <= 0) return fail(m, VDR_ERR_INVALID, "vdr_set_input_size: width must be positive");
  if (!m) return fail(m, VDR_ERR_INVALID, "vdr_set_input_size: null handle");
  const vdr_config& c = m->cfg;
  if (!c.patch) return fail(m, VDR_ERR_UNSUPPORTED, "vdr_set_input_size: image models only (token model)");
  if (c.window > 0)
    return fail(m, VDR_ERR_UNSUPPORTED,
                "vdr_set_input_size: not for the SAM encoder (its position tables and window partition are tied to its grid)");
  if (!c.pre_ln && c.layers > 0) return fail(m, VDR_ERR_UNSUPPORTED, "vdr_set_input_size: pre-LN models only");
  if (height % c.patch) return fail(m, VDR_ERR_INVALID, "vdr_set_input_size: height must be a multiple of patch " + std::to_string(c.patch));
  if (width % c.patch) return fail(m, VDR_ERR_INVALID, "vdr_set_input_size: width must be a multiple of patch " + std::to_string(c.patch));
  if ((int64_t)((height - c.patch) / m->stride + 1) * ((width - c.patch) / m->stride + 1) > (1 << 20))
    return fail(m, VDR_ERR_INVALID, "vdr_set_input_size: height x width gives more than 2^20 patches");
  int rc = check_device(m);
  if (rc) return rc;
  if (!m->resolved) return fail(m, VDR_ERR_INCOMPLETE, "vdr_set_input_size: vdr_finalize has not run since the last vdr_set_weight");
  DeviceGuard dg(m->device);
  if (!dg.ok) return fail(m, VDR_ERR_HIP, "hipSetDevice failed");
  return change_geometry(m, height, width, m->stride);
}

int vdr_set_patch_stride(vdr_handle m, int stride) {
  // the argument check that needs no handle comes first (it also holds for a null one)
  if (stride <= 0) return fail(m, VDR_ERR_INVALID, "vdr_set_patch_stride: stride must be positive");
  if (!m) return fail(m, VDR_ERR_INVALID, "vdr_set_patch_stride: null handle");
  const vdr_config& c = m->cfg;
  if (c.patch && (stride > c.patch || c.patch % stride))
    return fail(m, VDR_ERR_INVALID, "vdr_set_patch_stride: stride must divide patch " + std::to_string(c.patch));
  if (c.window > 0)
    return fail(m, VDR_ERR_UNSUPPORTED,
                "vdr_set_patch_stride: not for the SAM encoder (its position tables and window partition are tied to its grid)");
  if (!c.patch) return fail(m, VDR_ERR_UNSUPPORTED, "vdr_set_patch_stride: image models only (token model)");
  if (!c.pre_ln && c.layers > 0) return fail(m, VDR_ERR_UNSUPPORTED, "vdr_set_patch_stride: pre-LN models only");
  if (m->rope)
    return fail(m, VDR_ERR_UNSUPPORTED,
                "vdr_set_patch_stride: not for rope = 1 (DINOv3's patch coordinates are defined for non-overlapping patches only)");
  if ((int64_t)((m->in_h - c.patch) / stride + 1) * ((m->in_w - c.patch) / stride + 1) > (1 << 20))
    return fail(m, VDR_ERR_INVALID, "vdr_set_patch_stride: the input size in force gives more than 2^20 patches at this stride");
  int rc = check_device(m);
  if (rc) return rc;
  if (!m->resolved) return fail(m, VDR_ERR_INCOMPLETE, "vdr_set_patch_stride: vdr_finalize has not run since the last vdr_set_weight");
  DeviceGuard dg(m->device);
  if (!dg.ok) return fail(m, VDR_ERR_HIP, "hipSetDevice failed");
  return change_geometry(m, m->in_h, m->in_w, stride);
}

int vdr_get_patch_stride(vdr_handle m, int* stride) {
  if (!m || !stride) return fail(m, VDR_ERR_INVALID, "vdr_get_patch_stride: null argument");
  *stride = m->stride;
  return VDR_OK;
}

int vdr_get_input_size(vdr_handle m, int* height, int* width) {
  if (!m || !height || !width) return fail(m, VDR_ERR_INVALID, "vdr_get_input_size: null argument");
  *height = m->in_h;
  *width = m->in_w;
  return VDR_OK;
}

int vdr_workspace_bytes(vdr_handle m, int batch, int seq, size_t* out) {
  if (!m || !out || batch <= 0) return fail(m, VDR_ERR_INVALID, "bad argument");
  const int ntok = m->cfg.patch ? m->n_tokens : seq + (m->cfg.has_cls ? 1 : 0);
  if (ntok <= 0) return fail(m, VDR_ERR_INVALID, "seq must be positive for a token model");
  DeviceGuard dg(m->device);  // (the default split counts rounds on the handle's device, as the forward will)
  *out = batch_plan(m, batch, ntok).bytes;
  return VDR_OK;
}

int vdr_batch_plan(vdr_handle m, int batch, int seq, int32_t* micro_batch, int32_t* parts, int32_t* streams) {
  if (!m || !micro_batch || !parts || !streams || batch <= 0) return fail(m, VDR_ERR_INVALID, "bad argument");
  const int ntok = m->cfg.patch ? m->n_tokens : seq + (m->cfg.has_cls ? 1 : 0);
  if (ntok <= 0) return fail(m, VDR_ERR_INVALID, "seq must be positive for a token model");
  DeviceGuard dg(m->device);
  const BatchPlan p = batch_plan(m, batch, ntok);
  *micro_batch = p.mb;
  *parts = p.parts;
  *streams = p.streams;
  return VDR_OK;
}

int vdr_forward(vdr_handle m, const void* images, int in_dtype, int batch, void* out, int out_mode, int out_dtype,
                void* workspace, size_t workspace_bytes, void* stream) {
  if (!m || !images || !out || !workspace || batch <= 0) return fail(m, VDR_ERR_INVALID, "null/invalid argument");
  const vdr_config& c = m->cfg;
  if (!c.patch) return fail(m, VDR_ERR_INVALID, "vdr_forward needs an image model (patch > 0)");
  if (in_dtype != VDR_F32 && in_dtype != VDR_BF16) return fail(m, VDR_ERR_INVALID, "in_dtype");
  if (out_dtype != VDR_F32 && out_dtype != VDR_BF16) return fail(m, VDR_ERR_INVALID, "out_dtype");
  if (out_mode < VDR_OUT_CLS || out_mode > VDR_OUT_ENCODER) return fail(m, VDR_ERR_INVALID, "out_mode");
  if (out_mode == VDR_OUT_CLS && !c.has_cls) return fail(m, VDR_ERR_INVALID, "model has no cls token");
  if ((out_mode == VDR_OUT_ENCODER) != (c.window > 0 && out_mode != VDR_OUT_PATCH_EMBED && out_mode != VDR_OUT_TOKENS))
    return fail(m, VDR_ERR_INVALID, "VDR_OUT_ENCODER is the output of a SAM encoder (window > 0); other models use CLS/DENSE/TOKENS");
  const int ntok = m->n_tokens, n = m->n_patches, D = c.dim;
  const size_t img_bytes = (size_t)c.in_chans * m->in_h * m->in_w * (in_dtype == VDR_BF16 ? 2 : 4);
  const size_t es = out_dtype == VDR_BF16 ? 2 : 4;
  vdr_layer_out o{};  // (the output of the last block, as vdr_forward_layers describes one)
  o.out_mode = out_mode;
  o.out_dtype = out_dtype;
  o.norm = c.pre_ln ? 1 : 0;
  o.out = out;
  return run_micro_batches(m, batch, ntok, workspace, workspace_bytes, stream, [&](hipStream_t s, const Carve& w, int b0, int mb) {
    const char* img = (const char*)images + (size_t)b0 * img_bytes;
    if (out_mode == VDR_OUT_PATCH_EMBED) return embed_patches(m, s, w, img, in_dtype, mb, (char*)out + (size_t)b0 * n * D * es, out_dtype);
    int rc;
    if ((rc = embed_patches(m, s, w, img, in_dtype, mb, nullptr, out_dtype))) return rc;
    if (c.window > 0) {
      const bool tok = out_mode == VDR_OUT_TOKENS;
      return run_sam(m, s, w, mb, out_dtype, (char*)out + (size_t)b0 * n * (tok ? D : c.neck_chans) * es, tok);
    }
    if ((rc = assemble_stream(m, s, w, mb, ntok))) return rc;
    BlockRun r;
    r.cls_tail = out_mode == VDR_OUT_CLS;
    if ((rc = run_blocks(m, s, w, mb, ntok, r))) return rc;
    return write_output(m, s, w, mb, ntok, o, b0, r.compact);
  });
}

// vdr_forward_layers and vdr_forward_attn_maps (fn: the name the model refusals carry); the callers have checked the
// outs / maps arrays themselves
static int forward_layers_impl(const char* fn, vdr_handle m, const void* images, int in_dtype, int batch, const vdr_layer_out* outs,
                               int n_outs, const vdr_attn_map* maps, int n_maps, const vdr_facet_out* facets, int n_facets,
                               void* workspace, size_t workspace_bytes, void* stream) {
  for (int k = 0; k < n_outs; ++k) {
    const vdr_layer_out& o = outs[k];
    const std::string at = "outs[" + std::to_string(k) + "]: ";
    if (!o.out) return fail(m, VDR_ERR_INVALID, at + "null out");
    if (o.out_mode != VDR_OUT_CLS && o.out_mode != VDR_OUT_DENSE && o.out_mode != VDR_OUT_TOKENS && o.out_mode != VDR_OUT_POOLED)
      return fail(m, VDR_ERR_INVALID, at + "out_mode must be CLS, DENSE, TOKENS or POOLED");
    if (o.out_dtype != VDR_F32 && o.out_dtype != VDR_BF16) return fail(m, VDR_ERR_INVALID, at + "out_dtype");
    if (o.norm != 0 && o.norm != 1) return fail(m, VDR_ERR_INVALID, at + "norm must be 0 or 1");
    if (o.ld < 0) return fail(m, VDR_ERR_INVALID, at + "negative ld");
    if (o.ld != 0 && (o.out_mode == VDR_OUT_DENSE || o.out_mode == VDR_OUT_TOKENS))
      return fail(m, VDR_ERR_INVALID, at + "ld must be 0 for DENSE / TOKENS");
  }
  if (!m || !images || !workspace || batch <= 0) return fail(m, VDR_ERR_INVALID, "null/invalid argument");
  const vdr_config& c = m->cfg;
  if (!c.patch) return fail(m, VDR_ERR_UNSUPPORTED, std::string(fn) + ": image models only (token model)");
  if (c.window > 0) return fail(m, VDR_ERR_UNSUPPORTED, std::string(fn) + ": not for the SAM encoder (no final norm, a neck)");
  if (!c.pre_ln) return fail(m, VDR_ERR_UNSUPPORTED, std::string(fn) + ": pre-LN models only");
  if (c.layers <= 0) return fail(m, VDR_ERR_UNSUPPORTED, std::string(fn) + ": the model has no blocks");
  if (in_dtype != VDR_F32 && in_dtype != VDR_BF16) return fail(m, VDR_ERR_INVALID, "in_dtype");
  const int D = c.dim;
  EmitList el;
  el.at.resize(c.layers);
  el.maps.resize(c.layers);
  el.facets.resize(c.layers);
  for (int k = 0; k < n_facets; ++k) {
    const vdr_facet_out& f = facets[k];
    if (f.layer < 0 || f.layer >= c.layers)
      return fail(m, VDR_ERR_INVALID, "facets[" + std::to_string(k) + "]: layer " + std::to_string(f.layer) + " out of range 0.." +
                                          std::to_string(c.layers - 1));
    el.facets[f.layer].push_back(&f);
    if (f.layer > el.last) el.last = f.layer;
  }
  for (int k = 0; k < n_maps; ++k) {
    const vdr_attn_map& a = maps[k];
    const std::string at = "maps[" + std::to_string(k) + "]: ";
    if (a.layer < 0 || a.layer >= c.layers)
      return fail(m, VDR_ERR_INVALID, at + "layer " + std::to_string(a.layer) + " out of range 0.." + std::to_string(c.layers - 1));
    if (a.q_rows > m->n_tokens)
      return fail(m, VDR_ERR_INVALID, at + "q_rows " + std::to_string(a.q_rows) + " exceeds the " + std::to_string(m->n_tokens) + " tokens");
    el.maps[a.layer].push_back(&a);
    if (a.layer > el.last) el.last = a.layer;
  }
  for (int k = 0; k < n_outs; ++k) {
    const vdr_layer_out& o = outs[k];
    const std::string at = "outs[" + std::to_string(k) + "]: ";
    if (o.layer < 0 || o.layer >= c.layers)
      return fail(m, VDR_ERR_INVALID, at + "layer " + std::to_string(o.layer) + " out of range 0.." + std::to_string(c.layers - 1));
    if (o.out_mode == VDR_OUT_CLS && !c.has_cls) return fail(m, VDR_ERR_INVALID, at + "model has no cls token");
    if (o.ld != 0 && o.ld < D) return fail(m, VDR_ERR_INVALID, at + "ld must be 0 or >= D");
    el.at[o.layer].push_back(&o);
    if (o.layer > el.last) el.last = o.layer;
  }
  // binned facets, before anything is launched: 16-byte chunks of D channels, and the level means of the largest
  // micro-batch -- (h - 1) * mb * n * D fp32 -- inside the fc1 activation buffer (carve: Mp * mlp_hidden bf16)
  // (in either form of the forward: split by default, or whole on a stream that is being captured)
  for (const bool linear_only : {false, true}) {
    DeviceGuard dg(m->device);
    const int mb = batch_plan(m, batch, m->n_tokens, linear_only).mb;
    const size_t u_bytes = (size_t)carve(m, nullptr, mb, m->n_tokens).Mp * c.mlp_hidden * 2;
    for (int k = 0; k < n_facets; ++k) {
      const int h = facets[k].hierarchy;
      if (!h) continue;
      const std::string at = "facets[" + std::to_string(k) + "]: ";
      if (D % 8) return fail(m, VDR_ERR_UNSUPPORTED, at + "log-binning needs dim % 8 == 0");
      if ((size_t)(h - 1) * mb * m->n_patches * D * 4 > u_bytes)
        return fail(m, VDR_ERR_UNSUPPORTED, at + "the level means of hierarchy " + std::to_string(h) + " do not fit the MLP activation buffer");
    }
  }
  bool cls_only = true;  // every output of the last block that runs is CLS: that block may run its CLS rows only
  for (const vdr_layer_out* o : el.at[el.last]) cls_only = cls_only && o->out_mode == VDR_OUT_CLS;
  for (const vdr_facet_out* f : el.facets[el.last]) cls_only = cls_only && f->facet != VDR_FACET_TOKEN;  // (the stream's every row)
  const int ntok = m->n_tokens;
  const size_t img_bytes = (size_t)c.in_chans * m->in_h * m->in_w * (in_dtype == VDR_BF16 ? 2 : 4);
  return run_micro_batches(m, batch, ntok, workspace, workspace_bytes, stream, [&](hipStream_t s, const Carve& w, int b0, int mb) {
    int rc;
    if ((rc = embed_patches(m, s, w, (const char*)images + (size_t)b0 * img_bytes, in_dtype, mb, nullptr, VDR_F32))) return rc;
    if ((rc = assemble_stream(m, s, w, mb, ntok))) return rc;
    el.b0 = b0;
    BlockRun r;
    r.cls_tail = cls_only;
    r.el = &el;
    return run_blocks(m, s, w, mb, ntok, r);
  });
}

int vdr_forward_layers(vdr_handle m, const void* images, int in_dtype, int batch, const vdr_layer_out* outs, int n_outs,
                       void* workspace, size_t workspace_bytes, void* stream) {
  // argument checks that need no model first (they also hold for a null handle), then the model's
  if (!outs || n_outs <= 0) return fail(m, VDR_ERR_INVALID, "null outs or n_outs <= 0");
  return forward_layers_impl("vdr_forward_layers", m, images, in_dtype, batch, outs, n_outs, nullptr, 0, nullptr, 0, workspace,
                             workspace_bytes, stream);
}

// the per-map checks that need no model (vdr_forward_attn_maps, vdr_forward_facets)
static int check_maps(vdr_handle m, const vdr_attn_map* maps, int n_maps) {
  for (int k = 0; k < n_maps; ++k) {
    const vdr_attn_map& a = maps[k];
    const std::string at = "maps[" + std::to_string(k) + "]: ";
    if (!a.out) return fail(m, VDR_ERR_INVALID, at + "null out");
    if (a.q_rows < 1) return fail(m, VDR_ERR_INVALID, at + "q_rows must be >= 1");
    if (a.head_mean != 0 && a.head_mean != 1) return fail(m, VDR_ERR_INVALID, at + "head_mean must be 0 or 1");
    if (a.out_dtype != VDR_F32 && a.out_dtype != VDR_BF16) return fail(m, VDR_ERR_INVALID, at + "out_dtype");
  }
  return VDR_OK;
}

int vdr_forward_attn_maps(vdr_handle m, const void* images, int in_dtype, int batch, const vdr_layer_out* outs, int n_outs,
                          const vdr_attn_map* maps, int n_maps, void* workspace, size_t workspace_bytes, void* stream) {
  // the checks that need no model come first, as vdr_forward_layers orders its own
  if (!maps || n_maps <= 0) return fail(m, VDR_ERR_INVALID, "null maps or n_maps <= 0");
  if (int rc = check_maps(m, maps, n_maps)) return rc;
  if (n_outs < 0 || (n_outs > 0 && !outs)) return fail(m, VDR_ERR_INVALID, "null outs with n_outs > 0, or n_outs < 0");
  return forward_layers_impl("vdr_forward_attn_maps", m, images, in_dtype, batch, outs, n_outs, maps, n_maps, nullptr, 0, workspace,
                             workspace_bytes, stream);
}

int vdr_forward_facets(vdr_handle m, const void* images, int in_dtype, int batch, const vdr_layer_out* outs, int n_outs,
                       const vdr_attn_map* maps, int n_maps, const vdr_facet_out* facets, int n_facets, void* workspace,
                       size_t workspace_bytes, void* stream) {
  if (!facets || n_facets <= 0) return fail(m, VDR_ERR_INVALID, "null facets or n_facets <= 0");
  for (int k = 0; k < n_facets; ++k) {
    const vdr_facet_out& f = facets[k];
    const std::string at = "facets[" + std::to_string(k) + "]: ";
    if (!f.out) return fail(m, VDR_ERR_INVALID, at + "null out");
    if (f.facet < VDR_FACET_TOKEN || f.facet > VDR_FACET_VALUE) return fail(m, VDR_ERR_INVALID, at + "facet must be TOKEN, QUERY, KEY or VALUE");
    if (f.hierarchy < 0 || f.hierarchy > 3) return fail(m, VDR_ERR_INVALID, at + "hierarchy must be 0 (no binning) or 1..3");
    if (f.all_rows != 0 && f.all_rows != 1) return fail(m, VDR_ERR_INVALID, at + "all_rows must be 0 or 1");
    if (f.all_rows && f.hierarchy) return fail(m, VDR_ERR_INVALID, at + "a binned facet takes the patch rows only (all_rows = 0)");
    if (f.out_dtype != VDR_F32 && f.out_dtype != VDR_BF16) return fail(m, VDR_ERR_INVALID, at + "out_dtype");
  }
  if (n_outs < 0 || (n_outs > 0 && !outs)) return fail(m, VDR_ERR_INVALID, "null outs with n_outs > 0, or n_outs < 0");
  if (n_maps < 0 || (n_maps > 0 && !maps)) return fail(m, VDR_ERR_INVALID, "null maps with n_maps > 0, or n_maps < 0");
  if (int rc = check_maps(m, maps, n_maps)) return rc;
  return forward_layers_impl("vdr_forward_facets", m, images, in_dtype, batch, outs, n_outs, maps, n_maps, facets, n_facets, workspace,
                             workspace_bytes, stream);
}

static int forward_tokens_impl(vdr_handle m, const void* tokens, int in_dtype, int batch, int seq, const int32_t* seq_lens,
                               void* out, int out_mode, int out_dtype, void* workspace, size_t workspace_bytes, void* stream) {
  if (!m || !tokens || !out || !workspace || batch <= 0 || seq <= 0) return fail(m, VDR_ERR_INVALID, "null/invalid argument");
  const vdr_config& c = m->cfg;
  if (c.patch) return fail(m, VDR_ERR_INVALID, "vdr_forward_tokens needs a token model (patch == 0)");
  if (in_dtype != VDR_F32 && in_dtype != VDR_BF16) return fail(m, VDR_ERR_INVALID, "in_dtype");
  if (out_dtype != VDR_F32 && out_dtype != VDR_BF16) return fail(m, VDR_ERR_INVALID, "out_dtype");
  if (out_mode != VDR_OUT_CLS && out_mode != VDR_OUT_TOKENS && out_mode != VDR_OUT_DENSE)
    return fail(m, VDR_ERR_INVALID, "out_mode");
  if (out_mode == VDR_OUT_CLS && !c.has_cls) return fail(m, VDR_ERR_INVALID, "model has no cls token");
  const int ncls = c.has_cls ? 1 : 0;
  const int ntok = seq + ncls, D = c.dim;
  const size_t in_es = in_dtype == VDR_BF16 ? 2 : 4;
  vdr_layer_out o{};  // (the output of the last block, as vdr_forward_layers describes one)
  o.out_mode = out_mode;
  o.out_dtype = out_dtype;
  o.norm = c.pre_ln ? 1 : 0;
  o.out = out;
  return run_micro_batches(m, batch, ntok, workspace, workspace_bytes, stream, [&](hipStream_t s, const Carve& w, int b0, int mb) {
    const char* tok = (const char*)tokens + (size_t)b0 * seq * D * in_es;
    const int64_t M = (int64_t)mb * ntok;
    int rc;
    if (c.input_ln) {
      // LayerNorm([cls ; tokens]) straight from the caller's buffer (models_archs.py:143-145)
      const RowMap im = c.has_cls ? RowMap{ntok, seq, -1} : identity_map();
      if ((rc = layernorm(m, s, VDR_K_ASSEMBLE, tok, in_dtype == VDR_BF16, w.x, 1, m->inw, m->inb, M, im,
                          c.has_cls ? m->cls : nullptr, ntok)))
        return rc;
    } else {
      Scope sc(m, s, VDR_K_ASSEMBLE, 0.0, (double)M * D * (in_es + 2));
      VDR_TRY(launch_assemble_tokens(tok, in_dtype == VDR_BF16, m->cls, nullptr, w.x, mb, seq, D, ncls, s), "assemble");
    }
    BlockRun r;
    r.lens = seq_lens ? seq_lens + b0 : nullptr;
    r.len_add = ncls;
    if ((rc = run_blocks(m, s, w, mb, ntok, r))) return rc;
    return write_output(m, s, w, mb, ntok, o, b0, false);
  });
}

int vdr_forward_tokens(vdr_handle m, const void* tokens, int in_dtype, int batch, int seq, void* out, int out_mode,
                       int out_dtype, void* workspace, size_t workspace_bytes, void* stream) {
  return forward_tokens_impl(m, tokens, in_dtype, batch, seq, nullptr, out, out_mode, out_dtype, workspace, workspace_bytes, stream);
}

int vdr_forward_tokens_varlen(vdr_handle m, const void* tokens, int in_dtype, int batch, int max_seq, const int32_t* seq_lens,
                              void* out, int out_mode, int out_dtype, void* workspace, size_t workspace_bytes, void* stream) {
  if (!seq_lens) return fail(m, VDR_ERR_INVALID, "seq_lens is null");
  return forward_tokens_impl(m, tokens, in_dtype, batch, max_seq, seq_lens, out, out_mode, out_dtype, workspace, workspace_bytes,
                             stream);
}

// ---- single operators -----------------------------------------------------------------------------
// An entry point refuses what it cannot run (VDR_ERR_INVALID / VDR_ERR_UNSUPPORTED, vdr_last_error(NULL) = "<op>: <what>")
// BEFORE check_device, so every refusal is reachable without a GPU; then RUN_OP launches.  The descriptor ops (nn_cosine,
// affinity_bits, the PCA three, the Gram side, k-means, mahalanobis) describe their map as a DescOperand and share
// check_desc_operand; each adds only what it alone asks.  There is no kernel and no launch of its own in this file.
#define OP_TRY(expr, what)                                                             \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess) return fail(nullptr, VDR_ERR_HIP, std::string(what) + ": " + hipGetErrorString(_e)); \
  } while (0)

// an op that is one launch, as the LAST statement of its entry point: RETURNS FROM THE CALLER with the device check's
// refusal, with VDR_ERR_HIP "<what>: <HIP's text>" if the launch fails, else with VDR_OK
#define RUN_OP(launch, what)                       \
  do {                                             \
    if (int rc = check_device(nullptr)) return rc; \
    OP_TRY(launch, what);                          \
    return VDR_OK;                                 \
  } while (0)

// an op's GEMM: hipErrorInvalidValue is the caller's tile variant or shape (VDR_ERR_INVALID, `refused`)
static int op_gemm(const GemmArgs& g, int epilogue, int variant, void* stream, const char* refused) {
  const hipError_t e = launch_gemm(g, epilogue, variant, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) {
    (void)hipGetLastError();
    return fail(nullptr, VDR_ERR_INVALID, refused);
  }
  OP_TRY(e, "gemm");
  return VDR_OK;
}

// every pointer of the argument list on a 16-byte boundary (null: an absent optional argument)
static bool aligned16(std::initializer_list<const void*> ps) {
  uintptr_t u = 0;
  for (const void* q : ps) u |= (uintptr_t)q;
  return (u & 15) == 0;
}

// an op's refusal "<op>: <what>" as its return value
static int refuse(const char* op, int code, const std::string& what) { return fail(nullptr, code, std::string(op) + ": " + what); }

// The refusals the workspace ops and the mask-plane ops share, one per fact; each returns 0 when there is nothing to refuse.
static int refuse_workspace(const char* op, size_t have, size_t need) {
  return have < need ? refuse(op, VDR_ERR_WORKSPACE, "workspace too small: " + std::to_string(need) + " bytes needed") : 0;
}

// the plane count and the sides of a plane
static int refuse_planes(const char* op, int planes, int H, int W, int max_side) {
  if (planes < 1 || planes > 65535) return refuse(op, VDR_ERR_INVALID, "planes must be 1 .. 65535");
  if (H < 1 || H > max_side || W < 1 || W > max_side) return refuse(op, VDR_ERR_INVALID, "H and W must be 1 .. " + std::to_string(max_side));
  return 0;
}

// the logit planes of mask_stats and mask_binarize (include/vdr.h): sides, output size, the two strides
static int refuse_logit_planes(const char* op, int64_t plane_stride, int planes_per_group, int64_t group_stride, int planes, int H, int W, int oh,
                               int ow) {
  if (int rc = refuse_planes(op, planes, H, W, MS_MAX_SIDE)) return rc;
  if (oh < 1 || oh > MS_MAX_OUT || ow < 1 || ow > MS_MAX_OUT) return refuse(op, VDR_ERR_INVALID, "oh and ow must be 1 .. " + std::to_string(MS_MAX_OUT));
  if (plane_stride < (int64_t)H * W) return refuse(op, VDR_ERR_INVALID, "plane_stride is shorter than a plane");
  if (planes_per_group < 1 || planes % planes_per_group) return refuse(op, VDR_ERR_INVALID, "planes must be a multiple of planes_per_group >= 1");
  if (planes_per_group < planes && group_stride < (planes_per_group - 1) * plane_stride + (int64_t)H * W)
    return refuse(op, VDR_ERR_INVALID, "group_stride is shorter than a group's planes");
  return 0;
}

// A descriptor map as the descriptor ops take it (include/vdr.h): `problems` problems of `imgs` images of `t` rows of `d`
// channels, the rows `ld`, the images `image_stride`, the problems `problem_stride` elements apart.  An op without an image
// level passes imgs = 1 and image_stride = 0, one without a problem stride 0, a bf16-only op in_dtype = VDR_BF16.
// `packed`: a dense tensor that is read element by element and is no MFMA operand (window_vote's class scores): d is any
// positive count, and of the rows and strides nothing is asked -- only the base pointers are 16-byte aligned.
struct DescOperand {
  const void* x;
  int in_dtype;
  int64_t ld, image_stride, problem_stride;
  int problems, imgs, t, d;
  bool packed = false;
};
// what the op's signature calls the sizes, the row stride, the other strides and the row count of all problems
struct DescNames {
  const char *sizes, *ld, *strides, *rows;
};
static const DescNames PCA_NAMES = {"problems, imgs, t and d", "ld", "image_stride", "problems * R"};
static const DescNames GRAM_NAMES = {"problems, t and d", "ld", "image_stride", "problems * t"};
static const DescNames KMEANS_NAMES = {"problems, imgs, t and d", "ld", "the strides", "problems * R"};
static const DescNames NN_NAMES = {"pairs, tx, ty and d", "ldx and ldy", "the pair strides", "pairs * max(tx, ty)"};
static const DescNames KNN_NAMES = {"pairs, tq, tc and d", "ldx and ldy", "the pair strides", "pairs * max(tq, tc)"};
static const DescNames LOCAL_NAMES = {"pairs, gh, gw and d", "ldx and ldy", "the pair strides", "pairs * gh * gw"};
static const DescNames WINDOW_VOTE_NAMES = {"problems, sources, gh, gw and n_classes", "n_classes", "the strides",
                                            "problems * sources * gh * gw"};
static const DescNames AFFINITY_NAMES = {"pairs, t and d", "ldx", "x_stride", "pairs * t"};

// THE operand check of the descriptor ops, in one fixed order: dtype, null pointers, positive sizes, d % 32 (and d <= max_d
// where max_d > 0; not of a packed operand), ld >= d and strides >= 0, 16-byte alignment of x, of `required16` (the op's other
// pointers that must be non-null and 16-byte aligned), of the rows and of both strides (a packed operand: of the pointers
// alone), problems * imgs * t <= 2^31 - 1.  What only one op asks
// (k ranges, optional or 4-byte pointers, pitch, ...) stays in that op, after this.
static int check_desc_operand(const char* op, const DescOperand& o, const DescNames& n, int max_d,
                              std::initializer_list<const void*> required16) {
  if (o.in_dtype != VDR_F32 && o.in_dtype != VDR_BF16) return refuse(op, VDR_ERR_INVALID, "in_dtype must be VDR_F32 or VDR_BF16");
  bool null = !o.x;
  for (const void* q : required16) null = null || !q;
  if (null) return refuse(op, VDR_ERR_INVALID, "null pointer");
  if (o.problems <= 0 || o.imgs <= 0 || o.t <= 0 || o.d <= 0) return refuse(op, VDR_ERR_INVALID, std::string(n.sizes) + " must be positive");
  if (!o.packed && (o.d % 32 != 0 || (max_d > 0 && o.d > max_d)))
    return refuse(op, VDR_ERR_UNSUPPORTED, "d must be a multiple of 32" + (max_d > 0 ? ", at most " + std::to_string(max_d) : std::string()));
  if (o.ld < o.d || o.image_stride < 0 || o.problem_stride < 0) return refuse(op, VDR_ERR_INVALID, std::string(n.ld) + " must be >= d, " + n.strides + " >= 0");
  const int64_t per16 = o.in_dtype == VDR_BF16 ? 8 : 4;  // elements of a 16-byte chunk
  if (o.packed && (!aligned16({o.x}) || !aligned16(required16))) return refuse(op, VDR_ERR_INVALID, "pointers must be 16-byte aligned");
  if (!o.packed && (!aligned16({o.x}) || !aligned16(required16) || o.ld % per16 || o.image_stride % per16 || o.problem_stride % per16))
    return refuse(op, VDR_ERR_INVALID, std::string("pointers, rows (") + n.ld + ") and " + n.strides + " must be 16-byte aligned");
  const int64_t R = (int64_t)o.imgs * o.t;  // (each factor is a positive int: no overflow; R is bounded before the next product)
  if (R > INT32_MAX || R * o.problems > INT32_MAX) return refuse(op, VDR_ERR_INVALID, std::string(n.rows) + " exceeds 2^31 - 1");
  return VDR_OK;
}

int vdr_op_layernorm(const void* x, int in_dtype, void* y, int out_dtype, const float* gamma, const float* beta,
                     int64_t rows, int D, float eps, void* stream) {
  if (!x || !y || !gamma || !beta) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (rows <= 0) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_layernorm: rows must be positive");
  if (D <= 0 || (D & 3) || D > 2048)
    return fail(nullptr, VDR_ERR_UNSUPPORTED, "vdr_op_layernorm: D must be a positive multiple of 4, at most 2048");
  // a lane moves 4 elements per access: 8 bytes of bf16, 16 of fp32 (x, y); gamma and beta as f32x4
  if (((uintptr_t)x & (in_dtype == VDR_BF16 ? 7 : 15)) || ((uintptr_t)y & (out_dtype == VDR_BF16 ? 7 : 15)) || !aligned16({gamma, beta}))
    return fail(nullptr, VDR_ERR_INVALID, "vdr_op_layernorm: x / y must be aligned to 4 elements, gamma and beta to 16 bytes");
  if (int rc = check_device(nullptr)) return rc;
  LnArgs a{};
  a.x = x;
  a.in_bf16 = in_dtype == VDR_BF16;
  a.y = y;
  a.out_bf16 = out_dtype == VDR_BF16;
  a.gamma = gamma;
  a.beta = beta;
  a.rows = rows;
  a.D = D;
  a.eps = eps;
  a.imap = identity_map();
  a.omap = identity_map();
  OP_TRY(launch_layernorm(a, (hipStream_t)stream), "layernorm");
  return VDR_OK;
}

static int op_linear_impl(const void* x, const void* W, int packed, const float* bias, const void* resid, const float* gamma,
                          void* y, int64_t M, int N, int K, int epilogue, int variant, void* stream) {
  if (!x || !W || !y) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  // (the public activation values are the internal ones: vdr_kernels.h)
  static_assert((int)VDR_EPI_BIAS_QUICK_GELU == (int)EPI_BIAS_QGELU && (int)VDR_EPI_BIAS_GELU_TANH == (int)EPI_BIAS_TGELU, "vdr_epilogue");
  if ((epilogue < VDR_EPI_BIAS || epilogue > VDR_EPI_SWIGLU) && epilogue != VDR_EPI_BIAS_QUICK_GELU && epilogue != VDR_EPI_BIAS_GELU_TANH)
    return fail(nullptr, VDR_ERR_INVALID, "epilogue");
  if (epilogue == VDR_EPI_BIAS_RESID && !resid) return fail(nullptr, VDR_ERR_INVALID, "resid required");
  if (K % 64 || N % 8) return fail(nullptr, VDR_ERR_UNSUPPORTED, "K % 64 == 0 and N % 8 == 0 required");
#ifndef VDR_TUNING
  if (variant < 0 || variant >= 100) return fail(nullptr, VDR_ERR_INVALID, "variant");  // (ablation encodings: tuning builds only)
#endif
  // 16-byte operand loads (x, W), f32x4 bias / gamma, bf16x8 residual loads and output stores
  if (!aligned16({x, W, bias, resid, gamma, y}))
    return fail(nullptr, VDR_ERR_INVALID, "vdr_op_linear: x, W, bias, resid, gamma and y must be 16-byte aligned");
  if (int rc = check_device(nullptr)) return rc;
  GemmArgs g = linear(x, W, y, M, N, K, epilogue);
  g.w_interleaved = packed;
  g.bias = bias;
  g.resid = resid;
  g.gamma = gamma;
  if (variant == 0)  // library default: what the forward itself would pick for this shape
    variant = gemm_variant_for(N >= 2304 ? VDR_K_GEMM_QKV : VDR_K_GEMM_FC1, M, N);
  return op_gemm(g, epilogue, variant, stream, "gemm: unknown tile variant or unsupported shape");
}

int vdr_op_linear(const void* x, const void* W, const float* bias, const void* resid, const float* gamma, void* y,
                  int64_t M, int N, int K, int epilogue, int variant, void* stream) {
  return op_linear_impl(x, W, 0, bias, resid, gamma, y, M, N, K, epilogue, variant, stream);
}

int vdr_op_pack_linear_weight(const void* W, int N, int K, void* packed, void* stream) {
  if (!W || !packed) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (N <= 0 || (N & 1) || K <= 0 || (K & 31)) return fail(nullptr, VDR_ERR_UNSUPPORTED, "N even and K % 32 == 0 required");
  RUN_OP(launch_w_interleave(W, packed, N, K, K, (hipStream_t)stream),
         "w_interleave");
}

int vdr_op_linear_packed(const void* x, const void* Wp, const float* bias, const void* resid, const float* gamma, void* y,
                         int64_t M, int N, int K, int epilogue, int variant, void* stream) {
  return op_linear_impl(x, Wp, 1, bias, resid, gamma, y, M, N, K, epilogue, variant, stream);
}

// ---- the LayerNorm fold at op level: the forward's arithmetic (fold_ln_host, set_ln_fold, launch_gemm, launch_ln_finalize)
// on caller buffers
int vdr_ln_fold_weights(const float* W, const float* b, const float* gamma, const float* beta, int N, int K, int swiglu,
                        uint16_t* wf, float* colsum, float* tbias) {
  if (!W || !b || !gamma || !beta || !wf || !colsum || !tbias) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (N <= 0 || K <= 0 || (swiglu && (N % 64))) return fail(nullptr, VDR_ERR_INVALID, "N > 0, K > 0 (swiglu: N % 64 == 0) required");
  fold_ln_host(W, b, gamma, beta, N, K, swiglu != 0, wf, colsum, tbias);
  return VDR_OK;
}

static bool ln_variant_ok(int variant, bool allow_31) {
  return tile_variant(variant) && (allow_31 || variant != VARIANT_8P);
}

int vdr_op_linear_ln_stats(const void* x, const void* W, const float* bias, const void* resid, const float* gamma, void* y,
                           const float* resid32, float* y32, int64_t M, int N, int K, int variant, float* part,
                           int64_t part_stride, float* stats, uint32_t* counters, float eps, void* stream) {
  if (!x || !W || !y || !part || (!resid && !resid32)) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if ((resid32 != nullptr) != (y32 != nullptr)) return fail(nullptr, VDR_ERR_INVALID, "resid32 and y32 go together");
  if ((stats != nullptr) != (counters != nullptr)) return fail(nullptr, VDR_ERR_INVALID, "stats and counters go together");
  if (!ln_variant_ok(variant, false)) return fail(nullptr, VDR_ERR_INVALID, "variant: 22..29");
  if (stats && !ring4_variant(variant)) return fail(nullptr, VDR_ERR_INVALID, "in-GEMM finalisation: ring4 variants 26..29");
  if (M <= 0 || N <= 0 || K <= 0 || (N % 64) || (K % 64) || part_stride < M)
    return fail(nullptr, VDR_ERR_INVALID, "M > 0, N % 64 == 0, K % 64 == 0, part_stride >= M required");
  if (int rc = check_device(nullptr)) return rc;
  GemmArgs g = linear(x, W, y, M, N, K, EPI_BIAS_RESID);
  g.bias = bias;
  g.resid = resid ? resid : y;
  g.gamma = gamma;
  g.resid32 = resid32;
  g.C32 = y32;
  LnFold ln;
  ln.part = part;
  ln.part_stride = part_stride;
  ln.fin_stats = stats;
  ln.fin_cnt = counters;
  ln.eps = eps;
  set_ln_fold(g, ln);
  return op_gemm(g, EPI_BIAS_RESID, variant, stream, "gemm: unsupported tile variant or shape for the LayerNorm producer");
}

int vdr_op_ln_finalize(const float* part, int64_t part_stride, int64_t rows, int D, float eps, float* stats, void* stream) {
  if (!part || !stats) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (rows <= 0 || D <= 0 || (D % 64) || part_stride < rows)
    return fail(nullptr, VDR_ERR_INVALID, "rows > 0, D % 64 == 0, part_stride >= rows required");
  RUN_OP(launch_ln_finalize(part, D / 64, part_stride, stats, rows, D, eps, (hipStream_t)stream),
         "ln_finalize");
}

int vdr_op_linear_ln_fold(const void* x, const void* Wf, const float* colsum, const float* tbias, const float* stats,
                          const float* part, int64_t part_stride, void* y, int64_t M, int N, int K, int64_t x_rows, float eps,
                          int epilogue, int variant, void* stream) {
  if (!x || !Wf || !colsum || !tbias || !y) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if ((stats != nullptr) == (part != nullptr)) return fail(nullptr, VDR_ERR_INVALID, "exactly one of stats and part");
  if (epilogue != VDR_EPI_BIAS && !epi_is_act(epilogue) && epilogue != VDR_EPI_SWIGLU)
    return fail(nullptr, VDR_ERR_INVALID, "epilogue: bias, GELU / QuickGELU / tanh-GELU or SwiGLU");
  if (!ln_variant_ok(variant, true)) return fail(nullptr, VDR_ERR_INVALID, "variant: 22..29 or 31");
  if (M <= 0 || N <= 0 || K <= 0 || (N % 64) || (K % 64) || (x_rows && x_rows < M))
    return fail(nullptr, VDR_ERR_INVALID, "M > 0, N % 64 == 0, K % 64 == 0, x_rows 0 or >= M required");
  // (the forward finalises inside the GEMM on ring3 / ring4 variants 22-24, 26-28 only, up to 16 groups)
  if (part && (!ln_cpart_variant(variant) || K / 64 > 16 || part_stride < M))
    return fail(nullptr, VDR_ERR_INVALID, "in-GEMM statistics: variants 22-24, 26-28, K <= 1024, part_stride >= M");
  if (int rc = check_device(nullptr)) return rc;
  GemmArgs g = linear(x, Wf, y, M, N, K, epilogue);
  g.bias = tbias;
  g.a_rows = x_rows;
  LnFold ln;
  ln.stats = stats;
  ln.colsum = colsum;
  ln.cpart = part;
  ln.groups = K / 64;
  ln.cstride = part_stride;
  ln.eps = eps;
  set_ln_fold(g, ln);
  return op_gemm(g, epilogue, variant, stream, "gemm: unsupported tile variant or shape for the LayerNorm consumer");
}

size_t vdr_prepare_scratch_bytes(int batch, int h, int w, int channels, int out_side) {
  if (batch <= 0 || h <= 0 || w <= 0 || channels <= 0 || out_side <= 0) return 0;
  return prepare_scratch_bytes(batch, h, w, channels, out_side);
}

int vdr_op_prepare_image(const void* src, int src_dtype, int batch, int h, int w, int channels, int64_t stride_b,
                         int64_t stride_y, int64_t stride_x, int64_t stride_c, int flip, int out_side, void* out,
                         int out_dtype, void* scratch, void* stream) {
  if (!src || !out) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (src_dtype != VDR_F32 && src_dtype != VDR_F64) return fail(nullptr, VDR_ERR_UNSUPPORTED, "prepare_image: fp32 or fp64 input");
  if (out_dtype != VDR_F32 && out_dtype != VDR_BF16) return fail(nullptr, VDR_ERR_UNSUPPORTED, "prepare_image: fp32 or bf16 output");
  if (prepare_scratch_bytes(batch, h, w, channels, out_side) && !scratch)
    return fail(nullptr, VDR_ERR_INVALID, "prepare_image: down-scaling needs the scratch buffer");
  RUN_OP(launch_prepare(src, src_dtype == VDR_F32, batch, h, w, channels, stride_b, stride_y, stride_x, stride_c, flip,
                        out_side, out, out_dtype == VDR_BF16, (float*)scratch, (hipStream_t)stream),
         "prepare_image");
}

int vdr_op_window_ct(const void* ct, int in_dtype, int64_t n, double width, double level, float* out, void* stream) {
  if (!ct || !out) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (in_dtype != VDR_F32 && in_dtype != VDR_I16) return fail(nullptr, VDR_ERR_UNSUPPORTED, "window_ct: fp32 or int16 input");
  RUN_OP(launch_window_ct(ct, in_dtype == VDR_I16, n, width, level, out, (hipStream_t)stream),
         "window_ct");
}

int vdr_op_hu_to_rgb(const void* hu, int in_dtype, int64_t n, void* rgb, void* stream) {
  if (!hu || !rgb) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  const int dt = in_dtype == VDR_F32 ? 0 : in_dtype == VDR_I16 ? 1 : in_dtype == VDR_F64 ? 2 : -1;
  if (dt < 0) return fail(nullptr, VDR_ERR_UNSUPPORTED, "hu_to_rgb: fp32, int16 or fp64 input");
  RUN_OP(launch_hu_to_rgb(hu, dt, n, rgb, (hipStream_t)stream),
         "hu_to_rgb");
}

int vdr_op_crop_hwc(const float* src, float* dst, int batch, int H, int W, int C, int y0, int x0, int crop_h, int crop_w,
                    void* stream) {
  if (!src || !dst) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  RUN_OP(launch_crop_hwc(src, dst, batch, H, W, C, y0, x0, crop_h, crop_w, (hipStream_t)stream),
         "crop_hwc");
}

int vdr_op_voxel_sequence(const float* feat, const int64_t* index, const double* xyz, const double* expo, int64_t n, int D,
                          void* out, int out_dtype, void* stream) {
  if (n < 0 || D < 6) return fail(nullptr, VDR_ERR_INVALID, "voxel_sequence: n >= 0, D >= 6");
  if (n == 0) return VDR_OK;
  if (!feat || !index || !xyz || !expo || !out) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  const int dt = out_dtype == VDR_F32 ? 0 : out_dtype == VDR_BF16 ? 1 : out_dtype == VDR_F64 ? 2 : -1;
  if (dt < 0) return fail(nullptr, VDR_ERR_UNSUPPORTED, "voxel_sequence: fp32, bf16 or fp64 output");
  RUN_OP(launch_voxel_sequence(feat, index, xyz, expo, n, D, out, dt, (hipStream_t)stream),
         "voxel_sequence");
}

size_t vdr_affine_cubic_scratch_bytes(int h, int w, int64_t planes) {
  if (h <= 0 || w <= 0 || planes <= 0) return 0;
  return affine_cubic_scratch_bytes(h, w, planes);
}

int vdr_op_affine_cubic(const void* src, int dtype, int h, int w, int64_t planes, const double* matrix, const double* offset,
                        void* out, int clip01, void* scratch, void* stream) {
  if (!src || !out || !matrix || !offset || !scratch) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (h < 2 || w < 2 || planes <= 0) return fail(nullptr, VDR_ERR_INVALID, "affine_cubic: planes of at least 2 x 2");
  const int dt = dtype == VDR_F64 ? 0 : dtype == VDR_F32 ? 1 : dtype == VDR_U8 ? 2 : -1;
  if (dt < 0) return fail(nullptr, VDR_ERR_UNSUPPORTED, "affine_cubic: fp64, fp32 or uint8 (boolean mask) volume");
  if ((int64_t)(h + 24) * (w + 24) * planes >= ((int64_t)1 << 31) * 256)
    return fail(nullptr, VDR_ERR_UNSUPPORTED, "affine_cubic: volume too large for one launch");
  RUN_OP(launch_affine_cubic(src, dt, h, w, planes, matrix, offset, out, clip01, (double*)scratch, (hipStream_t)stream),
         "affine_cubic");
}

size_t vdr_mx_scale_bytes(int64_t rows, int K) { return rows > 0 && K > 0 ? mx_scale_bytes(rows, K) : 0; }

int vdr_op_mx_quantize(const void* x, int64_t rows, int K, void* q, void* scales, void* stream) {
  if (!x || !q || !scales) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  RUN_OP(launch_mx_quant(x, rows, K, K, q, scales, (hipStream_t)stream),
         "mx_quantize");
}

int vdr_op_mx_dequantize(const void* q, const void* scales, int64_t rows, int K, float* y, void* stream) {
  if (!q || !scales || !y) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  RUN_OP(launch_mx_dequant(q, scales, rows, K, y, (hipStream_t)stream),
         "mx_dequantize");
}

int vdr_op_layernorm_mx(const void* x, const float* gamma, const float* beta, float eps, int64_t rows, int D, void* q,
                        void* scales, void* stream) {
  if (!x || !gamma || !beta || !q || !scales) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  RUN_OP(launch_ln_mx(x, gamma, beta, eps, rows, D, q, scales, (hipStream_t)stream),
         "layernorm_mx");
}

int vdr_op_linear_mx(const void* xq, const void* xs, const void* wq, const void* ws, const float* bias, const void* resid,
                     const float* gamma, void* y, void* yscales, int64_t M, int N, int K, int epilogue, int variant,
                     void* stream) {
  if (!xq || !xs || !wq || !ws || !y) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (epilogue == VDR_EPI_BIAS_RESID && !resid) return fail(nullptr, VDR_ERR_INVALID, "EPI_BIAS_RESID needs resid");
  if (int rc = check_device(nullptr)) return rc;
  GemmArgs g = linear(xq, wq, y, M, N, K, epilogue);
  g.a_scale = xs;
  g.w_scale = ws;
  g.bias = bias;
  g.resid = resid;
  g.gamma = gamma;
  g.c_scale = yscales;
  OP_TRY(launch_gemm_mx(g, epilogue, variant, (hipStream_t)stream), "gemm_mx");
  return VDR_OK;
}

int vdr_op_attention(const void* qkv, void* out, int batch, int seq, int heads, int variant, void* stream) {
  if (!qkv || !out) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (batch <= 0 || seq <= 0 || heads <= 0) return fail(nullptr, VDR_ERR_INVALID, "bad shape");
  RUN_OP(launch_attention(qkv, out, batch, seq, heads, variant, (hipStream_t)stream),
         "attention");
}

int vdr_op_attention_hd(const void* qkv, void* out, int batch, int seq, int heads, int head_dim, int variant, void* stream) {
  if (!head_dim_ok(head_dim)) return fail(nullptr, VDR_ERR_UNSUPPORTED, "head dim must be 32, 64, 96 or 128");
  if (!qkv || !out) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (batch <= 0 || seq <= 0 || heads <= 0) return fail(nullptr, VDR_ERR_INVALID, "bad shape");
  RUN_OP(launch_attention(qkv, out, batch, seq, heads, variant, (hipStream_t)stream, nullptr, nullptr, 0, head_dim),
         "attention");
}

int vdr_op_attention_varlen(const void* qkv, void* out, int batch, int seq, int heads, int head_dim, const int32_t* lens,
                            int len_add, int variant, void* stream) {
  if (!head_dim_ok(head_dim)) return fail(nullptr, VDR_ERR_UNSUPPORTED, "head dim must be 32, 64, 96 or 128");
  if (!qkv || !out || !lens) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (batch <= 0 || seq <= 0 || heads <= 0) return fail(nullptr, VDR_ERR_INVALID, "bad shape");
  RUN_OP(launch_attention(qkv, out, batch, seq, heads, variant, (hipStream_t)stream, nullptr, lens, len_add, head_dim),
         "attention");
}

int vdr_op_attention_probs(const void* qkv, void* out, int batch, int seq, int heads, int head_dim, int q_rows, int head_mean,
                           int out_dtype, void* stream) {
  if (!head_dim_ok(head_dim)) return fail(nullptr, VDR_ERR_UNSUPPORTED, "head dim must be 32, 64, 96 or 128");
  if (!qkv || !out) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (batch <= 0 || seq <= 0 || heads <= 0) return fail(nullptr, VDR_ERR_INVALID, "bad shape");
  if (q_rows < 1 || q_rows > seq) return fail(nullptr, VDR_ERR_INVALID, "q_rows must be in [1, seq]");
  if (head_mean != 0 && head_mean != 1) return fail(nullptr, VDR_ERR_INVALID, "head_mean must be 0 or 1");
  if (out_dtype != VDR_F32 && out_dtype != VDR_BF16) return fail(nullptr, VDR_ERR_INVALID, "out_dtype");
  RUN_OP(launch_attention_probs(qkv, out, batch, seq, heads, head_dim, q_rows, head_mean, out_dtype == VDR_BF16,
                                (hipStream_t)stream),
         "attention_probs");
}

int vdr_op_attention_pool(const float* q, const void* kv, int64_t ldkv, void* out, int batch, int n, int heads, int head_dim,
                          void* stream) {
  if (!head_dim_ok(head_dim)) return fail(nullptr, VDR_ERR_UNSUPPORTED, "head dim must be 32, 64, 96 or 128");
  if (!q || !kv || !out) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (batch <= 0 || heads <= 0) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_attention_pool: batch and heads must be positive");
  if (n < 1) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_attention_pool: n must be at least 1");
  if ((int64_t)batch * heads > 0x7fffffff) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_attention_pool: more than 2^31 (image, head) pairs");
  if (ldkv < (int64_t)2 * heads * head_dim || (ldkv & 7))
    return fail(nullptr, VDR_ERR_INVALID, "vdr_op_attention_pool: ldkv must be a multiple of 8 and at least 2 * heads * head_dim");
  if ((uintptr_t)kv & 15) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_attention_pool: kv must be 16-byte aligned");
  RUN_OP(launch_attention_pool(q, kv, ldkv, out, batch, n, heads, head_dim, (hipStream_t)stream),
         "attention_pool");
}

// ---- the mask decoder ops (csrc/mask_decoder.hip) ----
int vdr_op_cross_attention(const void* q, int64_t ldq, const float* q_add, const void* k, int64_t ldk, const float* k_add,
                           const void* v, int64_t ldv, void* out, int64_t ldo, int problems, int tq, int tk, int heads,
                           int head_dim, void* stream) {
  const char* op = "vdr_op_cross_attention";
  if (!q || !k || !v || !out) return refuse(op, VDR_ERR_INVALID, "null pointer");
  if (head_dim != 16 && head_dim != 32) return refuse(op, VDR_ERR_UNSUPPORTED, "head dim must be 16 or 32");
  if (problems <= 0 || tq <= 0 || tk <= 0 || heads <= 0) return refuse(op, VDR_ERR_INVALID, "problems, tq, tk and heads must be positive");
  if (problems > 65535) return refuse(op, VDR_ERR_INVALID, "at most 65535 problems");
  if (tq > 16 && tk > 16) return refuse(op, VDR_ERR_UNSUPPORTED, "one of tq and tk must be at most 16");
  const int64_t HD = (int64_t)heads * head_dim;
  if (HD > 256) return refuse(op, VDR_ERR_UNSUPPORTED, "heads * head_dim must be at most 256");
  if (ldq < HD || ldk < HD || ldv < HD || ldo < HD || ((ldq | ldk | ldv | ldo) & 7))
    return refuse(op, VDR_ERR_INVALID, "ldq, ldk, ldv and ldo must be multiples of 8, at least heads * head_dim");
  if (!aligned16({q, q_add, k, k_add, v, out})) return refuse(op, VDR_ERR_INVALID, "pointers must be 16-byte aligned");
  RUN_OP(launch_cross_attention(q, ldq, q_add, k, ldk, k_add, v, ldv, out, ldo, problems, tq, tk, heads, head_dim, (hipStream_t)stream),
         "cross_attention");
}

int vdr_op_token_linear(const void* x, int64_t ldx, const void* x_add, int64_t ldxa, const void* W, const float* bias,
                        const void* resid, int64_t ldr, void* y, int out_dtype, int64_t ldy, int M, int N, int K, int groups,
                        int relu, void* stream) {
  const char* op = "vdr_op_token_linear";
  if (!x || !W || !y) return refuse(op, VDR_ERR_INVALID, "null pointer");
  if (out_dtype != VDR_F32 && out_dtype != VDR_BF16) return refuse(op, VDR_ERR_INVALID, "out_dtype must be VDR_F32 or VDR_BF16");
  if (M <= 0 || N <= 0 || K <= 0 || groups <= 0 || groups > M) return refuse(op, VDR_ERR_INVALID, "M, N, K must be positive, groups in [1, M]");
  if ((K & 7) || K > 2048) return refuse(op, VDR_ERR_UNSUPPORTED, "K must be a multiple of 8, at most 2048");
  if ((int64_t)((M + groups - 1) / groups + 7) / 8 * groups > 65535) return refuse(op, VDR_ERR_UNSUPPORTED, "too many rows");
  if (relu != 0 && relu != 1) return refuse(op, VDR_ERR_INVALID, "relu must be 0 or 1");
  if (ldx < K || (x_add && ldxa < K) || (resid && ldr < N) || ldy < N) return refuse(op, VDR_ERR_INVALID, "a leading dimension is shorter than its row");
  if (!aligned16({W}) || ((uintptr_t)x & 1) || ((uintptr_t)y & (out_dtype == VDR_F32 ? 3 : 1)) || ((uintptr_t)bias & 3))
    return refuse(op, VDR_ERR_INVALID, "W must be 16-byte aligned, the others to their element");
  RUN_OP(launch_token_linear(x, ldx, x_add, ldxa, W, bias, resid, ldr, y, out_dtype == VDR_F32, ldy, M, N, K, groups, relu,
                             (hipStream_t)stream),
         "token_linear");
}

int vdr_op_mask_upscale(const void* x, const void* W, const float* bias, const float* hyper, float* out, int problems, int g,
                        int gelu_in, void* stream) {
  const char* op = "vdr_op_mask_upscale";
  if (!x || !W || !bias || !hyper || !out) return refuse(op, VDR_ERR_INVALID, "null pointer");
  if (problems <= 0) return refuse(op, VDR_ERR_INVALID, "problems must be positive");
  if (g < 1 || g > 64) return refuse(op, VDR_ERR_UNSUPPORTED, "g must be in [1, 64]");
  if ((int64_t)problems * g * g * 4 > INT32_MAX) return refuse(op, VDR_ERR_INVALID, "problems * g * g * 4 exceeds 2^31 - 1");
  if (gelu_in != 0 && gelu_in != 1) return refuse(op, VDR_ERR_INVALID, "gelu_in must be 0 or 1");
  if (!aligned16({x, W, bias, hyper, out})) return refuse(op, VDR_ERR_INVALID, "pointers must be 16-byte aligned");
  RUN_OP(launch_mask_upscale(x, W, bias, hyper, out, problems, g, gelu_in, (hipStream_t)stream), "mask_upscale");
}

// ---- the mask prompt ops (csrc/mask_prompt.hip) ----
int vdr_op_mask_embed(const float* emb, int channels_last, const float* mask, int mask_per_image, const float* weights, void* keys,
                      int problems, int problems_per_image, int g, float eps, void* stream) {
  const char* op = "vdr_op_mask_embed";
  if (!emb || !mask || !weights || !keys) return refuse(op, VDR_ERR_INVALID, "null pointer");
  if ((channels_last != 0 && channels_last != 1) || (mask_per_image != 0 && mask_per_image != 1))
    return refuse(op, VDR_ERR_INVALID, "channels_last and mask_per_image must be 0 or 1");
  if (problems <= 0 || problems > 65535 || problems_per_image <= 0 || problems % problems_per_image)
    return refuse(op, VDR_ERR_INVALID, "problems must be 1 .. 65535 and a multiple of problems_per_image");
  if (g < 1 || g > 64) return refuse(op, VDR_ERR_UNSUPPORTED, "g must be in [1, 64]");
  if (!(eps > 0.0f)) return refuse(op, VDR_ERR_INVALID, "eps must be positive");
  if (!aligned16({emb, mask, weights, keys})) return refuse(op, VDR_ERR_INVALID, "pointers must be 16-byte aligned");
  RUN_OP(launch_mask_embed(emb, channels_last, mask, mask_per_image, weights, weights + MASK_EMBED_SMALL, weights + MASK_EMBED_SMALL + 16 * 256,
                           keys, problems, problems_per_image, g, eps, (hipStream_t)stream),
         "mask_embed");
}

int vdr_op_mask_box(const float* logits, int64_t plane_stride, const float* prev, float* boxes, int32_t* area, int problems, int H, int W,
                    int img, float margin, float threshold, void* stream) {
  const char* op = "vdr_op_mask_box";
  if (!logits || !prev || !boxes || !area) return refuse(op, VDR_ERR_INVALID, "null pointer");
  if (problems <= 0 || problems > 65535 || H <= 0 || W <= 0 || img <= 0) return refuse(op, VDR_ERR_INVALID, "problems (at most 65535), H, W and img must be positive");
  if ((int64_t)H * W > INT32_MAX) return refuse(op, VDR_ERR_UNSUPPORTED, "H * W exceeds 2^31 - 1");
  if (img > (1 << 24)) return refuse(op, VDR_ERR_UNSUPPORTED, "img must be exact in fp32: at most 2^24");
  if (plane_stride < (int64_t)H * W) return refuse(op, VDR_ERR_INVALID, "plane_stride is shorter than a plane");
  if (!(margin >= 0.0f) || threshold != threshold) return refuse(op, VDR_ERR_INVALID, "margin must be >= 0, threshold a number");
  if (((uintptr_t)logits & 3) || ((uintptr_t)area & 3) || !aligned16({prev, boxes})) return refuse(op, VDR_ERR_INVALID, "prev and boxes must be 16-byte aligned, the others to their element");
  RUN_OP(launch_mask_box(logits, plane_stride, prev, boxes, area, problems, H, W, (float)img, margin, threshold, (hipStream_t)stream), "mask_box");
}

// ---- the automatic mask generator's post-processing (csrc/mask_stats.hip, csrc/nms.hip) ----
size_t vdr_mask_stats_workspace_bytes(int planes, int H, int W, int oh, int ow) { return mask_stats_workspace_bytes(planes, H, W, oh, ow); }

int vdr_op_mask_stats(const float* logits, int64_t plane_stride, int planes_per_group, int64_t group_stride, int planes, int H, int W, int oh,
                      int ow, float threshold, float offset, void* workspace, size_t workspace_bytes, int32_t* counts, int32_t* box,
                      void* stream) {
  static_assert(VDR_MASK_STATS_MAX_SIDE == MS_MAX_SIDE && VDR_MASK_STATS_MAX_OUT == MS_MAX_OUT, "include/vdr.h and mask_stats_map.h");
  const char* op = "vdr_op_mask_stats";
  if (!logits || !workspace || !counts || !box) return refuse(op, VDR_ERR_INVALID, "null pointer");
  if (int rc = refuse_logit_planes(op, plane_stride, planes_per_group, group_stride, planes, H, W, oh, ow)) return rc;
  if (!(offset >= 0.0f)) return refuse(op, VDR_ERR_INVALID, "offset must be >= 0");
  if (((uintptr_t)logits & 3) || !aligned16({workspace, counts, box})) return refuse(op, VDR_ERR_INVALID, "workspace, counts and box must be 16-byte aligned, logits to its element");
  if (int rc = refuse_workspace(op, workspace_bytes, mask_stats_workspace_bytes(planes, H, W, oh, ow))) return rc;
  RUN_OP(launch_mask_stats(logits, plane_stride, planes_per_group, group_stride, planes, H, W, oh, ow, threshold, offset, workspace, counts, box,
                           (hipStream_t)stream),
         "mask_stats");
}

size_t vdr_nms_workspace_bytes(int n) { return nms_workspace_bytes(n); }

int vdr_op_nms(const float* boxes, const int32_t* order, int n, float iou_threshold, void* workspace, size_t workspace_bytes, uint8_t* keep,
               int32_t* kept, int32_t* count, void* stream) {
  static_assert(VDR_NMS_MAX_BOXES == NMS_MAX_BOXES, "include/vdr.h and vdr_kernels.h");
  const char* op = "vdr_op_nms";
  if (!boxes || !order || !workspace || !keep || !kept || !count) return refuse(op, VDR_ERR_INVALID, "null pointer");
  if (n < 1 || n > NMS_MAX_BOXES) return refuse(op, VDR_ERR_INVALID, "n must be 1 .. " + std::to_string(NMS_MAX_BOXES));
  if (iou_threshold != iou_threshold) return refuse(op, VDR_ERR_INVALID, "iou_threshold must be a number");
  if (!aligned16({boxes, workspace}) || (((uintptr_t)order | (uintptr_t)kept | (uintptr_t)count) & 3))
    return refuse(op, VDR_ERR_INVALID, "boxes and workspace must be 16-byte aligned, order, kept and count to their element");
  if (int rc = refuse_workspace(op, workspace_bytes, nms_workspace_bytes(n))) return rc;
  RUN_OP(launch_nms(boxes, order, n, iou_threshold, workspace, keep, kept, count, (hipStream_t)stream), "nms");
}

// ---- connected components of mask planes (csrc/components.hip) ----
size_t vdr_mask_binarize_workspace_bytes(int planes, int H, int W, int oh, int ow) { return mask_stats_workspace_bytes(planes, H, W, oh, ow) ? 16 : 0; }

int vdr_op_mask_binarize(const float* logits, int64_t plane_stride, int planes_per_group, int64_t group_stride, int planes, int H, int W, int oh,
                         int ow, float threshold, void* workspace, size_t workspace_bytes, uint8_t* out, void* stream) {
  const char* op = "vdr_op_mask_binarize";
  if (!logits || !workspace || !out) return refuse(op, VDR_ERR_INVALID, "null pointer");
  if (int rc = refuse_logit_planes(op, plane_stride, planes_per_group, group_stride, planes, H, W, oh, ow)) return rc;
  if (threshold != threshold) return refuse(op, VDR_ERR_INVALID, "threshold must be a number");
  if ((uintptr_t)logits & 3) return refuse(op, VDR_ERR_INVALID, "logits must be aligned to its element");
  if (int rc = refuse_workspace(op, workspace_bytes, vdr_mask_binarize_workspace_bytes(planes, H, W, oh, ow))) return rc;
  RUN_OP(launch_mask_binarize(logits, plane_stride, planes_per_group, group_stride, planes, H, W, oh, ow, threshold, out, (hipStream_t)stream),
         "mask_binarize");
}

size_t vdr_connected_components_workspace_bytes(int planes, int H, int W) { return components_workspace_bytes(planes, H, W, 0); }

int vdr_op_connected_components(const uint8_t* mask, int planes, int H, int W, int connectivity, int value, void* workspace, size_t workspace_bytes,
                                int32_t* root, int32_t* area, int32_t* count, void* stream) {
  static_assert(VDR_COMPONENTS_MAX_SIDE == CC_MAX_SIDE && CC_MAX_PLANES == 65535, "include/vdr.h and components_map.h");
  const char* op = "vdr_op_connected_components";
  if (!mask || !workspace || !root || !area || !count) return refuse(op, VDR_ERR_INVALID, "null pointer");
  if (int rc = refuse_planes(op, planes, H, W, CC_MAX_SIDE)) return rc;
  if (connectivity != 4 && connectivity != 8) return refuse(op, VDR_ERR_INVALID, "connectivity must be 4 or 8");
  if (value != 0 && value != 1) return refuse(op, VDR_ERR_INVALID, "value must be 0 or 1");
  if (!aligned16({workspace}) || (((uintptr_t)root | (uintptr_t)area | (uintptr_t)count) & 3))
    return refuse(op, VDR_ERR_INVALID, "workspace must be 16-byte aligned, root, area and count to their element");
  if (int rc = refuse_workspace(op, workspace_bytes, components_workspace_bytes(planes, H, W, 0))) return rc;
  RUN_OP(launch_connected_components(mask, planes, H, W, connectivity, value, workspace, root, area, count, (hipStream_t)stream),
         "connected_components");
}

size_t vdr_mask_clean_workspace_bytes(int planes, int H, int W) { return components_workspace_bytes(planes, H, W, 1); }

int vdr_op_mask_clean(const uint8_t* mask, int planes, int H, int W, int min_area, int connectivity, int mode, void* workspace,
                      size_t workspace_bytes, uint8_t* out, int32_t* changed, int32_t* stats, void* stream) {
  const char* op = "vdr_op_mask_clean";
  if (!mask || !workspace || !out || !changed || !stats) return refuse(op, VDR_ERR_INVALID, "null pointer");
  if (int rc = refuse_planes(op, planes, H, W, CC_MAX_SIDE)) return rc;
  if (connectivity != 4 && connectivity != 8) return refuse(op, VDR_ERR_INVALID, "connectivity must be 4 or 8");
  if (min_area < 0) return refuse(op, VDR_ERR_INVALID, "min_area must be >= 0");
  if (mode & ~(VDR_CLEAN_HOLES | VDR_CLEAN_ISLANDS | VDR_CLEAN_LARGEST)) return refuse(op, VDR_ERR_INVALID, "unknown mode bit");
  if ((mode & VDR_CLEAN_ISLANDS) && (mode & VDR_CLEAN_LARGEST)) return refuse(op, VDR_ERR_INVALID, "VDR_CLEAN_ISLANDS and VDR_CLEAN_LARGEST exclude each other");
  {
    const uintptr_t a = (uintptr_t)mask, b = (uintptr_t)out, n = (uintptr_t)planes * H * W;
    if (a < b + n && b < a + n) return refuse(op, VDR_ERR_INVALID, "out may not overlap mask");
  }
  if (!aligned16({workspace}) || (((uintptr_t)changed | (uintptr_t)stats) & 3))
    return refuse(op, VDR_ERR_INVALID, "workspace must be 16-byte aligned, changed and stats to their element");
  if (int rc = refuse_workspace(op, workspace_bytes, components_workspace_bytes(planes, H, W, 1))) return rc;
  RUN_OP(launch_mask_clean(mask, planes, H, W, min_area, connectivity, mode, workspace, out, changed, stats, (hipStream_t)stream), "mask_clean");
}

// ---- exact Euclidean distance transform of mask planes (csrc/edt.hip) ----
size_t vdr_distance_transform_workspace_bytes(int planes, int H, int W) { return distance_transform_workspace_bytes(planes, H, W); }

int vdr_op_distance_transform(const uint8_t* mask, int planes, int H, int W, int value, int outside, int r2, void* workspace, size_t workspace_bytes,
                              int32_t* d2, int32_t* nearest, int32_t* peak, uint8_t* within, void* stream) {
  static_assert(VDR_EDT_MAX_SIDE == EDT_MAX_SIDE && VDR_EDT_NONE == EDT_NONE && EDT_MAX_PLANES == 65535, "include/vdr.h and edt_map.h");
  const char* op = "vdr_op_distance_transform";
  if (!mask || !workspace) return refuse(op, VDR_ERR_INVALID, "null pointer");
  if (!d2 && !nearest && !peak && !within) return refuse(op, VDR_ERR_INVALID, "no output: d2, nearest, peak and within are all null");
  if (int rc = refuse_planes(op, planes, H, W, EDT_MAX_SIDE)) return rc;
  if (value != 0 && value != 1) return refuse(op, VDR_ERR_INVALID, "value must be 0 or 1");
  if (outside != 0 && outside != 1) return refuse(op, VDR_ERR_INVALID, "outside must be 0 or 1");
  if (nearest && outside) return refuse(op, VDR_ERR_INVALID, "nearest is not defined with outside = 1 (the nearest point may lie beyond the plane)");
  if (within && r2 < 0) return refuse(op, VDR_ERR_INVALID, "r2 must be >= 0");
  if (!aligned16({workspace}) || (((uintptr_t)d2 | (uintptr_t)nearest | (uintptr_t)peak) & 3))
    return refuse(op, VDR_ERR_INVALID, "workspace must be 16-byte aligned, d2, nearest and peak to their element");
  if (int rc = refuse_workspace(op, workspace_bytes, distance_transform_workspace_bytes(planes, H, W))) return rc;
  RUN_OP(launch_distance_transform(mask, planes, H, W, value, outside, r2, workspace, d2, nearest, peak, within, (hipStream_t)stream),
         "distance_transform");
}

// ---- exact 3-D Euclidean distance transform with integer voxel spacing (csrc/edt3d.hip) ----
size_t vdr_distance_transform_3d_workspace_bytes(int volumes, int Z, int H, int W) { return distance_transform_3d_workspace_bytes(volumes, Z, H, W); }

int vdr_op_distance_transform_3d(const uint8_t* vol, int volumes, int Z, int H, int W, int qz, int qy, int qx, int value, int outside, int64_t r2,
                                 void* workspace, size_t workspace_bytes, int64_t* d2, int64_t* peak, uint8_t* within, void* stream) {
  static_assert(VDR_EDT3_NONE == EDT3_NONE && VDR_EDT3_MAX_SPACING == EDT3_MAX_Q && VDR_EDT_MAX_SIDE == EDT_MAX_SIDE, "include/vdr.h and edt3d_map.h");
  const char* op = "vdr_op_distance_transform_3d";
  if (!vol || !workspace) return refuse(op, VDR_ERR_INVALID, "null pointer");
  if (!d2 && !peak && !within) return refuse(op, VDR_ERR_INVALID, "no output: d2, peak and within are all null");
  if (volumes < 1 || Z < 1 || Z > EDT_MAX_SIDE || H < 1 || H > EDT_MAX_SIDE || W < 1 || W > EDT_MAX_SIDE)
    return refuse(op, VDR_ERR_INVALID, "volumes must be >= 1, Z, H and W 1 .. " + std::to_string(EDT_MAX_SIDE));
  if ((int64_t)volumes * Z > EDT_MAX_PLANES) return refuse(op, VDR_ERR_INVALID, "volumes * Z must be at most 65535");
  if ((int64_t)Z * H * W > EDT3_MAX_VOXELS) return refuse(op, VDR_ERR_INVALID, "Z * H * W must be at most 2^30");
  if (qz < 1 || qz > EDT3_MAX_Q || qy < 1 || qy > EDT3_MAX_Q || qx < 1 || qx > EDT3_MAX_Q)
    return refuse(op, VDR_ERR_INVALID, "spacing must be three integers in 1 .. 65535");
  if (!edt3_spacing_ok(Z, H, W, qz, qy, qx))
    return refuse(op, VDR_ERR_INVALID, "(qz Z)^2 + (qy H)^2 + (qx W)^2 exceeds 2^53: distances would not be exact; use a coarser quantum");
  if (value != 0 && value != 1) return refuse(op, VDR_ERR_INVALID, "value must be 0 or 1");
  if (outside < 0 || outside > 7) return refuse(op, VDR_ERR_INVALID, "outside must be 0 .. 7 (bit 2 = z, bit 1 = y, bit 0 = x)");
  if (within && r2 < 0) return refuse(op, VDR_ERR_INVALID, "r2 must be >= 0");
  if (!aligned16({workspace}) || (((uintptr_t)d2 | (uintptr_t)peak) & 7))
    return refuse(op, VDR_ERR_INVALID, "workspace must be 16-byte aligned, d2 and peak to their element");
  if (int rc = refuse_workspace(op, workspace_bytes, distance_transform_3d_workspace_bytes(volumes, Z, H, W))) return rc;
  RUN_OP(launch_distance_transform_3d(vol, volumes, Z, H, W, qz, qy, qx, value, outside, r2, workspace, d2, peak, within, (hipStream_t)stream),
         "distance_transform_3d");
}

int vdr_op_attention_relpos(const void* qkv, const float* rel_pos_h, const float* rel_pos_w, float* rel, void* out,
                            int batch, int S, int heads, void* stream) {
  if (!qkv || !rel_pos_h || !rel_pos_w || !rel || !out) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (batch <= 0 || S <= 0 || heads <= 0) return fail(nullptr, VDR_ERR_INVALID, "bad shape");
  if (S > 64)
    return fail(nullptr, VDR_ERR_UNSUPPORTED, "vdr_op_attention_relpos: S must be at most 64 (the packed rel-pos operand holds 127 + 127 rows)");
  if (int rc = check_device(nullptr)) return rc;
  const int64_t tokens = (int64_t)batch * S * S;
  const int npad = relpos_npad(S);
  void* table = rel + tokens * heads * npad;  // packed bf16 tables behind the products
  OP_TRY(launch_relpos_pack(rel_pos_h, rel_pos_w, table, S, (hipStream_t)stream), "relpos_pack");
  OP_TRY(relpos_products(qkv, table, rel, tokens, S, heads, (hipStream_t)stream), "relpos");
  OP_TRY(launch_attention_relpos(qkv, rel, out, batch, S, heads, (hipStream_t)stream, env_int("VDR_RELPOS_ANY", 0)), "attention_relpos");
  return VDR_OK;
}

// ---- the SAM window path at op level: run_sam's own argument builders (sam_ln_args, sam_ln_mx, sam_proj_args) and launchers
// on caller buffers
// the kernels index rows with 32-bit arithmetic (g * g, the windowed row number)
static bool window_rows_ok(int batch, int g, int ws) {
  return g <= 32768 && ws <= 32768 && (int64_t)batch * sam_window_rows(g, ws) < ((int64_t)1 << 31);
}

int vdr_op_layernorm_window(const void* x, void* y, const float* gamma, const float* beta, int batch, int g, int ws, int D,
                            float eps, void* stream) {
  if (!x || !y || !gamma || !beta) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (batch < 1 || g < 1 || ws < 1) return fail(nullptr, VDR_ERR_INVALID, "bad shape");
  if (!window_rows_ok(batch, g, ws)) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_layernorm_window: more than 2^31 windowed rows");
  if (D <= 0 || (D & 3) || D > 2048)
    return fail(nullptr, VDR_ERR_UNSUPPORTED, "vdr_op_layernorm_window: D must be a positive multiple of 4, at most 2048");
  if (!aligned16({x, y, gamma, beta}))
    return fail(nullptr, VDR_ERR_INVALID, "vdr_op_layernorm_window: x, y, gamma and beta must be 16-byte aligned");
  RUN_OP(launch_layernorm(sam_ln_args(x, y, gamma, beta, eps, batch, g, ws, D), (hipStream_t)stream), "layernorm");
}

int vdr_op_layernorm_mx_window(const void* x, const float* gamma, const float* beta, float eps, int batch, int g, int ws, int D,
                               void* q, void* scales, void* stream) {
  if (!x || !gamma || !beta || !q || !scales) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (batch < 1 || g < 1 || ws < 1) return fail(nullptr, VDR_ERR_INVALID, "bad shape");
  if (!window_rows_ok(batch, g, ws)) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_layernorm_mx_window: more than 2^31 windowed rows");
  if (D <= 0 || (D & 31) || D > 2048)
    return fail(nullptr, VDR_ERR_UNSUPPORTED, "vdr_op_layernorm_mx_window: D must be a positive multiple of 32, at most 2048");
  if (!aligned16({x, gamma, beta, q}))
    return fail(nullptr, VDR_ERR_INVALID, "vdr_op_layernorm_mx_window: x, gamma, beta and q must be 16-byte aligned");
  RUN_OP(sam_ln_mx(x, gamma, beta, eps, batch, g, ws, D, q, scales, (hipStream_t)stream), "layernorm_mx");
}

int vdr_op_linear_window(const void* x, const void* W, const float* bias, const void* resid, void* y, int batch, int g, int ws,
                         int N, int K, int variant, float* part, int64_t part_stride, void* stream) {
  if (!x || !W || !resid || !y) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (batch < 1 || g < 1 || ws < 1) return fail(nullptr, VDR_ERR_INVALID, "bad shape");
  if (!window_rows_ok(batch, g, ws)) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_linear_window: more than 2^31 windowed rows");
  if (N <= 0 || K <= 0 || K % 64 || N % 8) return fail(nullptr, VDR_ERR_UNSUPPORTED, "K % 64 == 0 and N % 8 == 0 required");
  if (variant != 0 && !ln_variant_ok(variant, false)) return fail(nullptr, VDR_ERR_INVALID, "variant: 0 or 22..29");
  if (part && (N % 64 || part_stride < (int64_t)batch * g * g))
    return fail(nullptr, VDR_ERR_INVALID, "vdr_op_linear_window: part needs N % 64 == 0 and part_stride >= batch * g * g");
  if (!aligned16({x, W, bias, resid, y, part}))
    return fail(nullptr, VDR_ERR_INVALID, "vdr_op_linear_window: x, W, bias, resid, y and part must be 16-byte aligned");
  if (int rc = check_device(nullptr)) return rc;
  const GemmArgs ga = sam_proj_args(x, W, bias, resid, y, batch, g, ws, N, K, part, part_stride);
  if (variant == 0) variant = gemm_variant_for(VDR_K_GEMM_PROJ, ga.M, ga.N);  // (what run_sam launches the out-projection on)
  return op_gemm(ga, EPI_BIAS_RESID, variant, stream, "gemm: unknown tile variant or unsupported shape");
}

int vdr_op_im2col3(const void* x, void* col, int batch, int g, int C, void* stream) {
  if (!x || !col) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (batch < 1 || g < 1) return fail(nullptr, VDR_ERR_INVALID, "bad shape");
  if (!window_rows_ok(batch, g, 0)) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_im2col3: more than 2^31 rows");
  if (C <= 0 || (C & 7)) return fail(nullptr, VDR_ERR_UNSUPPORTED, "vdr_op_im2col3: C must be a positive multiple of 8");
  if (!aligned16({x, col})) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_im2col3: x and col must be 16-byte aligned");
  RUN_OP(launch_im2col3(x, col, batch, g, C, (hipStream_t)stream), "im2col3");
}

int vdr_op_interpolate_rel_pos(const float* table, int L0, int D, float* out, int L, void* stream) {
  if (!table) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_interpolate_rel_pos: table is null");
  if (!out) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_interpolate_rel_pos: out is null");
  if (L0 <= 0) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_interpolate_rel_pos: L0 must be positive");
  if (D <= 0) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_interpolate_rel_pos: D must be positive");
  if (L <= 0) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_interpolate_rel_pos: L must be positive");
  if ((int64_t)L0 * D > (1 << 30) || (int64_t)L * D > (1 << 30))
    return fail(nullptr, VDR_ERR_INVALID, "vdr_op_interpolate_rel_pos: more than 2^30 table elements");
  RUN_OP(launch_relpos_interp(table, L0, D, out, L, (hipStream_t)stream),
         "relpos_interp");
}

int vdr_op_interpolate_pos(const float* pos, int gh0, int gw0, int D, float* out, int gh, int gw, void* stream) {
  if (!pos) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_interpolate_pos: pos is null");
  if (!out) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_interpolate_pos: out is null");
  if (gh0 <= 0) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_interpolate_pos: gh0 must be positive");
  if (gw0 <= 0) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_interpolate_pos: gw0 must be positive");
  if (D <= 0) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_interpolate_pos: D must be positive");
  if (gh <= 0) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_interpolate_pos: gh must be positive");
  if (gw <= 0) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_interpolate_pos: gw must be positive");
  if ((int64_t)gh0 * gw0 > (1 << 20) || (int64_t)gh * gw > (1 << 20))
    return fail(nullptr, VDR_ERR_INVALID, "vdr_op_interpolate_pos: more than 2^20 grid cells");
  RUN_OP(launch_pos_interp(pos, gh0, gw0, D, out, gh, gw, (hipStream_t)stream),
         "pos_interp");
}

int vdr_op_rope2d_table(int gh, int gw, int head_dim, float theta, float* cos_out, float* sin_out, void* stream) {
  if (head_dim != 32 && head_dim != 64 && head_dim != 128)
    return fail(nullptr, VDR_ERR_UNSUPPORTED, "vdr_op_rope2d_table: head_dim must be 32, 64 or 128");
  if (!cos_out || !sin_out) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_rope2d_table: null table");
  if (gh <= 0 || gw <= 0 || (int64_t)gh * gw > (1 << 20))
    return fail(nullptr, VDR_ERR_INVALID, "vdr_op_rope2d_table: gh, gw must be positive, at most 2^20 grid cells");
  if (!(std::isfinite(theta) && theta > 1.0f)) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_rope2d_table: theta must be finite and > 1");
  RUN_OP(launch_rope2d_table(gh, gw, head_dim, theta, cos_out, sin_out, (hipStream_t)stream),
         "rope2d_table");
}

int vdr_op_rope2d(void* qkv, int batch, int seq, int prefix, int heads, int head_dim, const float* cos, const float* sin,
                  void* stream) {
  if (head_dim != 32 && head_dim != 64 && head_dim != 128)
    return fail(nullptr, VDR_ERR_UNSUPPORTED, "vdr_op_rope2d: head_dim must be 32, 64 or 128");
  if (!qkv || !cos || !sin) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_rope2d: null argument");
  if (batch <= 0 || seq <= 0 || heads <= 0 || prefix < 0 || prefix > seq)
    return fail(nullptr, VDR_ERR_INVALID, "vdr_op_rope2d: batch, seq, heads must be positive and 0 <= prefix <= seq");
  if ((((uintptr_t)qkv) | ((uintptr_t)cos) | ((uintptr_t)sin)) & 15)
    return fail(nullptr, VDR_ERR_INVALID, "vdr_op_rope2d: qkv, cos and sin must be 16-byte aligned");
  RUN_OP(launch_rope2d(qkv, batch, seq, prefix, heads, head_dim, cos, sin, (hipStream_t)stream),
         "rope2d");
}

int vdr_op_patch_embed(const void* images, int in_dtype, const void* W, const float* bias, const float* pos, void* col,
                       void* y, int batch, int C, int img, int p, int D, int row_stride, int row_offset, void* stream) {
  if (!images || !W || !col || !y) return fail(nullptr, VDR_ERR_INVALID, "null argument");
  if (p <= 0 || img % p) return fail(nullptr, VDR_ERR_INVALID, "img must be a multiple of p");
  if (int rc = check_device(nullptr)) return rc;
  GemmArgs a;
  int variant;  // (the caller's W as it is; bf16 images with p = 8 / 16 / 32: no im2col pass, `col` untouched)
  OP_TRY(patch_gemm(nullptr, (hipStream_t)stream, images, in_dtype, col, W, y, batch, C, img, img, p, p, D, &a, &variant), "im2col");
  a.bias = bias;
  a.pos = pos;
  a.omap = RowMap{(img / p) * (img / p), row_stride, row_offset};
  OP_TRY(launch_gemm(a, EPI_PATCH, variant, (hipStream_t)stream), "patch gemm");
  return VDR_OK;
}

int vdr_op_patch_embed_strided(const void* images, int in_dtype, const void* W, const float* bias, const float* pos, void* col,
                               void* y, int batch, int C, int H, int Wd, int p, int stride, int D, int row_stride, int row_offset,
                               void* stream) {
  if (!images || !W || !col || !y) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_patch_embed_strided: null argument");
  if (in_dtype != VDR_F32 && in_dtype != VDR_BF16) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_patch_embed_strided: in_dtype");
  if (batch <= 0 || C <= 0 || D <= 0 || p <= 0) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_patch_embed_strided: batch, C, D and p must be positive");
  if (stride <= 0 || stride > p || p % stride)
    return fail(nullptr, VDR_ERR_INVALID, "vdr_op_patch_embed_strided: stride must be positive and divide p");
  if (H < p || Wd < p || (H - p) % stride || (Wd - p) % stride)
    return fail(nullptr, VDR_ERR_INVALID, "vdr_op_patch_embed_strided: (H - p) and (W - p) must be non-negative multiples of stride");
  const int64_t n = (int64_t)((H - p) / stride + 1) * ((Wd - p) / stride + 1);
  if (n > (1 << 20) || n * batch > INT32_MAX) return fail(nullptr, VDR_ERR_INVALID, "vdr_op_patch_embed_strided: more than 2^20 patches per image or 2^31 rows");
  if (int rc = check_device(nullptr)) return rc;
  GemmArgs a;
  int variant;  // (stride == p: vdr_op_patch_embed's paths, rectangular sizes through im2col)
  OP_TRY(patch_gemm(nullptr, (hipStream_t)stream, images, in_dtype, col, W, y, batch, C, H, Wd, p, stride, D, &a, &variant), "im2col");
  a.bias = bias;
  a.pos = pos;
  a.omap = RowMap{(int)n, row_stride, row_offset};
  OP_TRY(launch_gemm(a, EPI_PATCH, variant, (hipStream_t)stream), "patch gemm");
  return VDR_OK;
}

int vdr_op_log_bin(const void* x, int in_dtype, int64_t ld, int64_t image_stride, int batch, int gh, int gw, int C, int hierarchy,
                   float* work, void* out, int out_dtype, void* stream) {
  if ((in_dtype != VDR_F32 && in_dtype != VDR_BF16) || (out_dtype != VDR_F32 && out_dtype != VDR_BF16))
    return fail(nullptr, VDR_ERR_INVALID, "log_bin: dtype");
  if (!x || !out || batch <= 0 || gh <= 0 || gw <= 0 || C <= 0) return fail(nullptr, VDR_ERR_INVALID, "log_bin: null pointer or non-positive size");
  if (hierarchy < 1 || hierarchy > 3) return fail(nullptr, VDR_ERR_UNSUPPORTED, "log_bin: hierarchy must be 1, 2 or 3");
  if (C % 8 != 0) return fail(nullptr, VDR_ERR_INVALID, "log_bin: C must be a multiple of 8");
  if (ld < C || image_stride < 0) return fail(nullptr, VDR_ERR_INVALID, "log_bin: ld must be >= C, image_stride >= 0");
  if (hierarchy > 1 && !work) return fail(nullptr, VDR_ERR_INVALID, "log_bin: null work with hierarchy > 1");
  const int64_t per16 = in_dtype == VDR_BF16 ? 8 : 4;  // elements of a 16-byte chunk
  if (!aligned16({x, out, work}) || ld % per16 || image_stride % per16)
    return fail(nullptr, VDR_ERR_INVALID, "log_bin: x, work, out and every row (ld, image_stride) must be 16-byte aligned");
  if ((int64_t)batch * gh * gw > INT32_MAX) return fail(nullptr, VDR_ERR_INVALID, "log_bin: batch * gh * gw exceeds 2^31 - 1");
  RUN_OP(launch_log_bin(x, in_dtype == VDR_BF16, ld, image_stride, batch, gh, gw, C, hierarchy, work, out, out_dtype == VDR_BF16,
                        (hipStream_t)stream),
         "log_bin");
}

size_t vdr_nn_cosine_work_bytes(int pairs, int tx, int ty) { return nn_cosine_work_bytes(pairs, tx, ty); }

int vdr_op_nn_cosine(const void* x, int64_t ldx, int64_t x_stride, int tx, const void* y, int64_t ldy, int64_t y_stride, int ty,
                     int pairs, int d, void* work, float* row_sim, int32_t* row_idx, float* col_sim, int32_t* col_idx,
                     void* stream) {
  if (int rc = check_desc_operand("nn_cosine", {x, VDR_BF16, ldx, 0, x_stride, pairs, 1, tx, d}, NN_NAMES, 0, {work, row_sim, row_idx}))
    return rc;
  if (int rc = check_desc_operand("nn_cosine", {y, VDR_BF16, ldy, 0, y_stride, pairs, 1, ty, d}, NN_NAMES, 0, {})) return rc;
  if (!col_sim != !col_idx) return refuse("nn_cosine", VDR_ERR_INVALID, "col_sim and col_idx must both be given or both be null");
  if (!aligned16({col_sim, col_idx})) return refuse("nn_cosine", VDR_ERR_INVALID, "col_sim and col_idx must be 16-byte aligned");
  RUN_OP(launch_nn_cosine(x, ldx, x_stride, tx, y, ldy, y_stride, ty, pairs, d, work, row_sim, row_idx, col_sim, col_idx,
                          (hipStream_t)stream),
         "nn_cosine");
}

size_t vdr_knn_work_bytes(int pairs, int tq, int tc, int k) { return knn_work_bytes(pairs, tq, tc, k); }

int vdr_op_knn(const void* x, int64_t ldx, int64_t x_stride, int tq, const void* y, int64_t ldy, int64_t y_stride, int tc, int pairs,
               int d, int k, int metric, int exclude_diag, void* work, float* val, int32_t* idx, void* stream) {
  static_assert(VDR_KNN_MAX_K == KNN_MAX_K, "include/vdr.h and knn_map.h");
  const char* op = "knn";
  if (int rc = check_desc_operand(op, {x, VDR_BF16, ldx, 0, x_stride, pairs, 1, tq, d}, KNN_NAMES, 0, {work, val, idx})) return rc;
  if (int rc = check_desc_operand(op, {y, VDR_BF16, ldy, 0, y_stride, pairs, 1, tc, d}, KNN_NAMES, 0, {})) return rc;
  if (k < 1 || k > VDR_KNN_MAX_K)
    return refuse(op, VDR_ERR_UNSUPPORTED, "k must be 1 .. " + std::to_string(VDR_KNN_MAX_K) + " (larger lists are out of scope)");
  if (metric != VDR_KNN_COSINE && metric != VDR_KNN_L2) return refuse(op, VDR_ERR_INVALID, "metric must be VDR_KNN_COSINE or VDR_KNN_L2");
  if ((int64_t)tc - (exclude_diag ? 1 : 0) < k) return refuse(op, VDR_ERR_INVALID, "fewer than k eligible candidates (tc - exclude_diag < k)");
  if ((int64_t)pairs * tq > INT32_MAX / k) return refuse(op, VDR_ERR_INVALID, "pairs * tq * k exceeds 2^31 - 1");
  RUN_OP(launch_knn(x, ldx, x_stride, tq, y, ldy, y_stride, tc, pairs, d, k, metric == VDR_KNN_L2, exclude_diag, work, val, idx,
                    (hipStream_t)stream),
         "knn");
}

size_t vdr_local_correlation_work_bytes(int pairs, int gh, int gw, int radius) {
  return local_correlation_work_bytes(pairs, gh, gw, radius);
}

int vdr_op_local_correlation(const void* x, int64_t ldx, int64_t x_stride, const void* y, int64_t ldy, int64_t y_stride, int pairs,
                             int gh, int gw, int d, int radius, int transposed, void* work, float* cost, float* best_sim,
                             int32_t* best_idx, void* stream) {
  static_assert(VDR_LOCAL_CORR_MAX_RADIUS == LC_MAX_RADIUS, "include/vdr.h and local_corr_map.h");
  const char* op = "local_correlation";
  // t as check_desc_operand takes it: 0 for a grid that is not positive (its refusal), capped where gh * gw overflows (ours, below)
  const int64_t t64 = gh > 0 && gw > 0 ? (int64_t)gh * gw : 0;
  const int t = (int)(t64 > INT32_MAX ? INT32_MAX : t64);
  if (int rc = check_desc_operand(op, {x, VDR_BF16, ldx, 0, x_stride, pairs, 1, t, d}, LOCAL_NAMES, 0, {work})) return rc;
  if (int rc = check_desc_operand(op, {y, VDR_BF16, ldy, 0, y_stride, pairs, 1, t, d}, LOCAL_NAMES, 0, {})) return rc;
  if (t64 > INT32_MAX) return refuse(op, VDR_ERR_INVALID, "gh * gw exceeds 2^31 - 1");
  if (radius < 1 || radius > VDR_LOCAL_CORR_MAX_RADIUS)
    return refuse(op, VDR_ERR_UNSUPPORTED, "radius must be 1 .. " + std::to_string(VDR_LOCAL_CORR_MAX_RADIUS));
  if (!cost && !best_sim && !best_idx) return refuse(op, VDR_ERR_INVALID, "no output: give cost, or best_sim and best_idx, or all three");
  if (!best_sim != !best_idx) return refuse(op, VDR_ERR_INVALID, "best_sim and best_idx must both be given or both be null");
  if (!aligned16({cost, best_sim, best_idx})) return refuse(op, VDR_ERR_INVALID, "cost, best_sim and best_idx must be 16-byte aligned");
  const int64_t WW = (int64_t)(2 * radius + 1) * (2 * radius + 1);
  if ((int64_t)pairs * t > INT32_MAX / WW) return refuse(op, VDR_ERR_INVALID, "pairs * gh * gw * (2 radius + 1)^2 exceeds 2^31 - 1");
  RUN_OP(launch_local_correlation(x, ldx, x_stride, y, ldy, y_stride, pairs, gh, gw, d, radius, transposed, work, cost, best_sim,
                                  best_idx, (hipStream_t)stream),
         "local_correlation");
}

int vdr_op_window_vote(const float* cost, const float* src, int problems, int sources, int gh, int gw, int radius, int k,
                       int n_classes, int weights, float temperature, float* scores, int32_t* labels, int32_t* idx, float* val,
                       void* stream) {
  const char* op = "window_vote";
  // t as in vdr_op_local_correlation: 0 for a grid that is not positive, capped where gh * gw overflows (refused below)
  const int64_t t64 = gh > 0 && gw > 0 ? (int64_t)gh * gw : 0;
  const int t = (int)(t64 > INT32_MAX ? INT32_MAX : t64);
  if (int rc = check_desc_operand(op, {src, VDR_F32, n_classes, 0, 0, problems, sources, t, n_classes, true}, WINDOW_VOTE_NAMES, 0,
                                  {cost, scores}))
    return rc;
  if (t64 > INT32_MAX) return refuse(op, VDR_ERR_INVALID, "gh * gw exceeds 2^31 - 1");
  if (sources > VDR_WINDOW_VOTE_MAX_SOURCES)
    return refuse(op, VDR_ERR_UNSUPPORTED, "sources must be 1 .. " + std::to_string(VDR_WINDOW_VOTE_MAX_SOURCES));
  if (radius < 1 || radius > VDR_LOCAL_CORR_MAX_RADIUS)
    return refuse(op, VDR_ERR_UNSUPPORTED, "radius must be 1 .. " + std::to_string(VDR_LOCAL_CORR_MAX_RADIUS));
  if (k < 1 || k > VDR_WINDOW_VOTE_MAX_K) return refuse(op, VDR_ERR_UNSUPPORTED, "k must be 1 .. " + std::to_string(VDR_WINDOW_VOTE_MAX_K));
  if (n_classes > VDR_WINDOW_VOTE_MAX_CLASSES)
    return refuse(op, VDR_ERR_UNSUPPORTED, "n_classes must be 1 .. " + std::to_string(VDR_WINDOW_VOTE_MAX_CLASSES));
  const int corner = sources * std::min(gh, radius + 1) * std::min(gw, radius + 1);
  if (k > corner)
    return refuse(op, VDR_ERR_INVALID, "k exceeds the " + std::to_string(corner) + " in-grid candidates of a corner patch, sources * min(gh, radius + 1) * min(gw, radius + 1)");
  if (weights != VDR_VOTE_SOFTMAX && weights != VDR_VOTE_UNIFORM)
    return refuse(op, VDR_ERR_INVALID, "weights must be VDR_VOTE_SOFTMAX or VDR_VOTE_UNIFORM");
  if (!(temperature > 0.f) || !std::isfinite(temperature)) return refuse(op, VDR_ERR_INVALID, "temperature must be positive and finite");
  if (!idx != !val) return refuse(op, VDR_ERR_INVALID, "idx and val must both be given or both be null");
  if (!aligned16({labels, idx, val})) return refuse(op, VDR_ERR_INVALID, "labels, idx and val must be 16-byte aligned");
  const int64_t rows = (int64_t)problems * sources * t, WW = (int64_t)(2 * radius + 1) * (2 * radius + 1);
  if (rows > INT32_MAX / WW) return refuse(op, VDR_ERR_INVALID, "problems * sources * gh * gw * (2 radius + 1)^2 exceeds 2^31 - 1");
  if (rows > INT32_MAX / n_classes) return refuse(op, VDR_ERR_INVALID, "problems * sources * gh * gw * n_classes exceeds 2^31 - 1");
  // (idx and val have fewer elements than cost: k <= sources * (radius + 1)^2 < sources * (2 radius + 1)^2)
  RUN_OP(launch_window_vote(cost, src, problems, sources, gh, gw, radius, k, n_classes, weights, temperature, scores, labels, idx, val,
                            (hipStream_t)stream),
         "window_vote");
}

size_t vdr_affinity_work_bytes(int pairs, int t) { return affinity_work_bytes(pairs, t); }

int vdr_op_affinity_bits(const void* x, int64_t ldx, int64_t x_stride, int t, int pairs, int d, float tau, int exclude_diag,
                         void* work, uint32_t* bits, int pitch, void* stream) {
  if (int rc = check_desc_operand("affinity_bits", {x, VDR_BF16, ldx, 0, x_stride, pairs, 1, t, d}, AFFINITY_NAMES, 0, {work, bits}))
    return rc;
  if (pitch != affinity_pitch(t)) return fail(nullptr, VDR_ERR_INVALID, "affinity_bits: pitch must be ceil(t / 32) rounded up to a multiple of 4");
  if (!(tau == tau)) return fail(nullptr, VDR_ERR_INVALID, "affinity_bits: tau is NaN");
  RUN_OP(launch_affinity_bits(x, ldx, x_stride, t, pairs, d, tau, exclude_diag, work, bits, pitch, (hipStream_t)stream), "affinity_bits");
}

int vdr_op_bits_matvec(const uint32_t* bits, int pitch, int t, int pairs, const float* v, int nv, float* y, int32_t* degree,
                       void* stream) {
  if (!bits || !v || !y) return fail(nullptr, VDR_ERR_INVALID, "bits_matvec: null bits, v or y");
  if (pairs <= 0 || t <= 0) return fail(nullptr, VDR_ERR_INVALID, "bits_matvec: pairs and t must be positive");
  if (nv < 1 || nv > 8) return fail(nullptr, VDR_ERR_UNSUPPORTED, "bits_matvec: nv must be 1 .. 8");
  if (!aligned16({bits}) || ((uintptr_t)v | (uintptr_t)y | (uintptr_t)degree) % 4)
    return fail(nullptr, VDR_ERR_INVALID, "bits_matvec: bits must be 16-byte aligned, v, y and degree 4-byte aligned");
  if ((int64_t)pairs * t > INT32_MAX) return fail(nullptr, VDR_ERR_INVALID, "bits_matvec: pairs * t exceeds 2^31 - 1");
  if (pitch != affinity_pitch(t)) return fail(nullptr, VDR_ERR_INVALID, "bits_matvec: pitch must be ceil(t / 32) rounded up to a multiple of 4");
  RUN_OP(launch_bits_matvec(bits, pitch, t, pairs, v, nv, y, degree, (hipStream_t)stream), "bits_matvec");
}

size_t vdr_pca_work_bytes(int problems, int imgs, int t, int d) { return pca_work_bytes(problems, imgs, t, d); }

int vdr_op_col_mean(const void* x, int in_dtype, int64_t ld, int64_t image_stride, int problems, int imgs, int t, int d, void* work,
                    float* mean, void* stream) {
  if (int rc = check_desc_operand("col_mean", {x, in_dtype, ld, image_stride, 0, problems, imgs, t, d}, PCA_NAMES, 2048, {work, mean})) return rc;
  RUN_OP(launch_col_mean(x, in_dtype == VDR_BF16, ld, image_stride, problems, imgs, t, d, work, mean, (hipStream_t)stream), "col_mean");
}

int vdr_op_covariance(const void* x, int in_dtype, int64_t ld, int64_t image_stride, int problems, int imgs, int t, int d,
                      const float* mean, void* work, float* cov, void* stream) {
  if (int rc = check_desc_operand("covariance", {x, in_dtype, ld, image_stride, 0, problems, imgs, t, d}, PCA_NAMES, 2048, {mean, work, cov})) return rc;
  if ((int64_t)imgs * t < 2) return fail(nullptr, VDR_ERR_INVALID, "covariance: needs R = imgs * t >= 2 rows");
  RUN_OP(launch_covariance(x, in_dtype == VDR_BF16, ld, image_stride, problems, imgs, t, d, mean, work, cov, (hipStream_t)stream),
         "covariance");
}

int vdr_op_pca_project(const void* x, int in_dtype, int64_t ld, int64_t image_stride, int problems, int imgs, int t, int d,
                       const float* mean, const float* comps, int k, int scale, void* work, float* proj, float* minmax,
                       void* stream) {
  if (int rc = check_desc_operand("pca_project", {x, in_dtype, ld, image_stride, 0, problems, imgs, t, d}, PCA_NAMES, 2048,
                                  {mean, comps, work, proj, minmax}))
    return rc;
  if (k < 1 || k > 8) return fail(nullptr, VDR_ERR_UNSUPPORTED, "pca_project: k must be 1..8");
  RUN_OP(launch_pca_project(x, in_dtype == VDR_BF16, ld, image_stride, problems, imgs, t, d, mean, comps, k, scale, work, proj,
                            minmax, (hipStream_t)stream),
         "pca_project");
}

size_t vdr_pca_topk_work_bytes(int problems, int t, int d, int k) {
  const size_t side = pca_topk_side_work_bytes(problems, t, d, k), solver = sym_topk_work_bytes(problems, t);
  return side > solver ? side : solver;
}

int vdr_op_col_mean_any(const void* x, int in_dtype, int64_t ld, int64_t image_stride, int problems, int t, int d, void* work,
                        float* mean, void* stream) {
  if (int rc = check_desc_operand("col_mean_any", {x, in_dtype, ld, image_stride, 0, problems, 1, t, d}, GRAM_NAMES, 0, {work, mean})) return rc;
  RUN_OP(launch_col_mean_any(x, in_dtype == VDR_BF16, ld, image_stride, problems, t, d, work, mean, (hipStream_t)stream), "col_mean_any");
}

int vdr_op_gram(const void* x, int in_dtype, int64_t ld, int64_t image_stride, int problems, int t, int d, const float* mean,
                void* work, float* gram, void* stream) {
  if (int rc = check_desc_operand("gram", {x, in_dtype, ld, image_stride, 0, problems, 1, t, d}, GRAM_NAMES, 0, {mean, work, gram})) return rc;
  if (t < 2 || t > 4096) return fail(nullptr, VDR_ERR_UNSUPPORTED, "gram: t must be 2..4096");
  RUN_OP(launch_gram(x, in_dtype == VDR_BF16, ld, image_stride, problems, t, d, mean, work, gram, (hipStream_t)stream), "gram");
}

int vdr_op_pca_back_project(const void* x, int in_dtype, int64_t ld, int64_t image_stride, int problems, int t, int d,
                            const float* mean, const float* u, const float* values, int k, void* work, float* comps, void* stream) {
  if (int rc = check_desc_operand("pca_back_project", {x, in_dtype, ld, image_stride, 0, problems, 1, t, d}, GRAM_NAMES, 0,
                                  {mean, u, values, work, comps}))
    return rc;
  if (k < 1 || k > 8) return fail(nullptr, VDR_ERR_UNSUPPORTED, "pca_back_project: k must be 1..8");
  RUN_OP(launch_pca_back_project(x, in_dtype == VDR_BF16, ld, image_stride, problems, t, d, mean, u, values, k, work, comps,
                                 (hipStream_t)stream),
         "pca_back_project");
}

int vdr_op_sym_topk(const float* a, int problems, int n, int k, float tol, int max_iter, void* work, float* values, float* vectors,
                    int32_t* iters, float* resid, void* stream) {
  if (!a || !work || !values || !vectors || !iters || !resid) return fail(nullptr, VDR_ERR_INVALID, "sym_topk: null pointer");
  if (problems <= 0) return fail(nullptr, VDR_ERR_INVALID, "sym_topk: problems must be positive");
  if (n < 2 || n > 4096) return fail(nullptr, VDR_ERR_UNSUPPORTED, "sym_topk: n must be 2..4096");
  if (k < 1 || k > 8 || k > n) return fail(nullptr, VDR_ERR_UNSUPPORTED, "sym_topk: k must be 1..min(8, n)");
  if (!(tol >= 0.0f) || max_iter < 1) return fail(nullptr, VDR_ERR_INVALID, "sym_topk: tol must be >= 0, max_iter >= 1");
  if (!aligned16({a, work, values, vectors, iters, resid}))
    return fail(nullptr, VDR_ERR_INVALID, "sym_topk: pointers must be 16-byte aligned");
  RUN_OP(launch_sym_topk(a, problems, n, k, tol, max_iter, work, values, vectors, iters, resid, (hipStream_t)stream), "sym_topk");
}

size_t vdr_kmeans_work_bytes(int problems, int imgs, int t, int d, int k) { return kmeans_work_bytes(problems, imgs, t, d, k); }

// what the two k-means ops ask beyond the operand check (include/vdr.h)
static int kmeans_own(const char* op, int imgs, int t, int k, const void* active) {
  if (k < 1 || k > 1024) return refuse(op, VDR_ERR_UNSUPPORTED, "k must be 1..1024");
  if (!aligned16({active})) return refuse(op, VDR_ERR_INVALID, "active must be 16-byte aligned");
  if (k > (int64_t)imgs * t) return refuse(op, VDR_ERR_INVALID, "k exceeds the R = imgs * t rows of a problem");
  return VDR_OK;
}

int vdr_op_kmeans_assign(const void* x, int64_t ld, int64_t image_stride, int64_t problem_stride, int problems, int imgs, int t,
                         int d, int k, const float* centroids, const int32_t* active, void* work, int32_t* labels, float* min_dist,
                         float* inertia, int32_t* changed, void* stream) {
  if (int rc = check_desc_operand("kmeans_assign", {x, VDR_BF16, ld, image_stride, problem_stride, problems, imgs, t, d}, KMEANS_NAMES, 0,
                                  {centroids, work, labels, min_dist, inertia, changed}))
    return rc;
  if (int rc = kmeans_own("kmeans_assign", imgs, t, k, active)) return rc;
  RUN_OP(launch_kmeans_assign(x, ld, image_stride, problem_stride, problems, imgs, t, d, k, centroids, active, work, labels,
                              min_dist, inertia, changed, (hipStream_t)stream),
         "kmeans_assign");
}

int vdr_op_kmeans_update(const void* x, int64_t ld, int64_t image_stride, int64_t problem_stride, int problems, int imgs, int t,
                         int d, int k, const int32_t* labels, const int32_t* active, void* work, float* centroids, int32_t* counts,
                         void* stream) {
  if (int rc = check_desc_operand("kmeans_update", {x, VDR_BF16, ld, image_stride, problem_stride, problems, imgs, t, d}, KMEANS_NAMES, 0,
                                  {labels, work, centroids, counts}))
    return rc;
  if (int rc = kmeans_own("kmeans_update", imgs, t, k, active)) return rc;
  RUN_OP(launch_kmeans_update(x, ld, image_stride, problem_stride, problems, imgs, t, d, k, labels, active, work, centroids, counts,
                              (hipStream_t)stream),
         "kmeans_update");
}

int vdr_op_mahalanobis(const void* x, int64_t ld, int64_t image_stride, int64_t problem_stride, int problems, int imgs, int t, int d,
                       const float* mean, int64_t mean_stride, const float* whiten, int64_t whiten_stride, int k, float* d2,
                       void* stream) {
  if (int rc = check_desc_operand("mahalanobis", {x, VDR_BF16, ld, image_stride, problem_stride, problems, imgs, t, d}, KMEANS_NAMES, 0,
                                  {mean, whiten}))
    return rc;
  if (!d2) return refuse("mahalanobis", VDR_ERR_INVALID, "null pointer");
  if (k < 1 || k > VDR_MAHALANOBIS_MAX_K) return refuse("mahalanobis", VDR_ERR_UNSUPPORTED, "k must be 1..2048");
  if ((mean_stride != 0 && mean_stride < d) || (whiten_stride != 0 && whiten_stride < (int64_t)k * d))
    return refuse("mahalanobis", VDR_ERR_INVALID, "mean_stride must be 0 or >= d, whiten_stride 0 or >= k * d");
  if ((uintptr_t)d2 % 4 || mean_stride % 4 || whiten_stride % 4)
    return refuse("mahalanobis", VDR_ERR_INVALID, "the model strides (mean_stride, whiten_stride) must be 16-byte aligned, d2 4-byte aligned");
  RUN_OP(launch_mahalanobis(x, ld, image_stride, problem_stride, problems, imgs, t, d, mean, mean_stride, whiten, whiten_stride, k, d2,
                            (hipStream_t)stream),
         "mahalanobis");
}

size_t vdr_upsample_work_bytes(int batch, int Cg, int gh, int gw) { return upsample_work_bytes(batch, Cg, gh, gw); }

// the guide and the geometry shared by the two upsampling ops (include/vdr.h); sets gh, gw
static int upsample_guide(const char* op, const void* guide, int guide_dtype, int batch, int Cg, int H, int W, int p, int s,
                          int* gh, int* gw) {
  const auto refuse = [op](int code, const char* what) { return ::refuse(op, code, what); };
  if (guide_dtype != VDR_F32 && guide_dtype != VDR_BF16) return refuse(VDR_ERR_INVALID, "guide_dtype must be VDR_F32 or VDR_BF16");
  if (!guide) return refuse(VDR_ERR_INVALID, "null guide");
  if (Cg < 1 || Cg > 4) return refuse(VDR_ERR_UNSUPPORTED, "the guide must have 1..4 channels");
  if (batch <= 0 || p <= 0 || s <= 0 || H <= 0 || W <= 0) return refuse(VDR_ERR_INVALID, "batch, patch, stride, H and W must be positive");
  if (p > 4096 || H > (1 << 24) || W > (1 << 24)) return refuse(VDR_ERR_INVALID, "patch above 4096 or a side above 2^24");
  if (p % s) return refuse(VDR_ERR_INVALID, "stride must divide patch");
  if (H < p || W < p || (H - p) % s || (W - p) % s)
    return refuse(VDR_ERR_INVALID, "H and W must be patch + (gh - 1) stride and patch + (gw - 1) stride");
  if ((uintptr_t)guide % (guide_dtype == VDR_BF16 ? 2 : 4)) return refuse(VDR_ERR_INVALID, "guide is not aligned to its element");
  *gh = (H - p) / s + 1;
  *gw = (W - p) / s + 1;
  if ((int64_t)batch * Cg * *gh * *gw > INT32_MAX) return refuse(VDR_ERR_INVALID, "batch * Cg * gh * gw exceeds 2^31 - 1");
  return VDR_OK;
}

int vdr_op_guide_lowres(const void* guide, int guide_dtype, int batch, int Cg, int H, int W, int p, int s, void* work, void* stream) {
  int gh, gw;
  if (int rc = upsample_guide("guide_lowres", guide, guide_dtype, batch, Cg, H, W, p, s, &gh, &gw)) return rc;
  if (!work || !aligned16({work})) return fail(nullptr, VDR_ERR_INVALID, "guide_lowres: work must be non-null and 16-byte aligned");
  RUN_OP(launch_guide_lowres(guide, guide_dtype == VDR_BF16, batch, Cg, H, W, p, s, gh, gw, (float*)work, (hipStream_t)stream),
         "guide_lowres");
}

int vdr_op_upsample_guided(const void* f, int f_dtype, int64_t ld, int64_t image_stride, int batch, int gh, int gw, int C,
                           const void* guide, int guide_dtype, int Cg, int H, int W, int p, int s, int radius, float cs, float cr,
                           const float* conf, int y0, int x0, int y1, int x1, void* work, void* out, int out_dtype, void* stream) {
  if ((f_dtype != VDR_F32 && f_dtype != VDR_BF16) || (out_dtype != VDR_F32 && out_dtype != VDR_BF16))
    return fail(nullptr, VDR_ERR_INVALID, "upsample_guided: dtype");
  if (!f || !work || !out) return fail(nullptr, VDR_ERR_INVALID, "upsample_guided: null features, work or out");
  if (radius < 1 || radius > 3) return fail(nullptr, VDR_ERR_UNSUPPORTED, "upsample_guided: radius must be 1, 2 or 3");
  int ggh, ggw;
  if (int rc = upsample_guide("upsample_guided", guide, guide_dtype, batch, Cg, H, W, p, s, &ggh, &ggw)) return rc;
  if (gh != ggh || gw != ggw)
    return fail(nullptr, VDR_ERR_INVALID, "upsample_guided: H and W must be patch + (gh - 1) stride and patch + (gw - 1) stride");
  if (C <= 0 || C % 8 != 0) return fail(nullptr, VDR_ERR_INVALID, "upsample_guided: C must be a positive multiple of 8");
  if (ld < C || image_stride < 0) return fail(nullptr, VDR_ERR_INVALID, "upsample_guided: ld must be >= C, image_stride >= 0");
  const int64_t per16 = f_dtype == VDR_BF16 ? 8 : 4;  // elements of a 16-byte chunk
  if (!aligned16({f, work, out}) || ld % per16 || image_stride % per16 || (uintptr_t)conf % 4)
    return fail(nullptr, VDR_ERR_INVALID,
                "upsample_guided: features, work, out and every row (ld, image_stride) must be 16-byte aligned, confidence 4-byte aligned");
  if (y0 < 0 || x0 < 0 || y1 > H || x1 > W || y0 >= y1 || x0 >= x1)
    return fail(nullptr, VDR_ERR_INVALID, "upsample_guided: the box must be non-empty and inside the image");
  if ((int64_t)(y1 - y0) * (x1 - x0) > INT32_MAX)
    return fail(nullptr, VDR_ERR_INVALID, "upsample_guided: the box has more than 2^31 - 1 pixels");
  if (!(cs >= 0.0f) || !(cr >= 0.0f) || cs > 3.0e38f || cr > 3.0e38f)
    return fail(nullptr, VDR_ERR_INVALID, "upsample_guided: cs and cr must be finite and >= 0");
  RUN_OP(launch_upsample_guided(f, f_dtype == VDR_BF16, ld, image_stride, batch, gh, gw, C, guide, guide_dtype == VDR_BF16, Cg, H, W, p,
                                s, radius, cs, cr, conf, y0, x0, y1, x1, (float*)work, out, out_dtype == VDR_BF16, (hipStream_t)stream),
         "upsample_guided");
}

// ---- profiler ---------------------------------------------------------------------------------------
int vdr_profile_enable(vdr_handle m, int on) {
  if (!m) return fail(m, VDR_ERR_INVALID, "null handle");
  m->prof = on != 0;
  return VDR_OK;
}

int vdr_profile_mask(vdr_handle m, uint32_t class_mask) {
  if (!m) return fail(m, VDR_ERR_INVALID, "null handle");
  m->prof_mask = class_mask;
  return VDR_OK;
}

int vdr_profile_read(vdr_handle m, double* ms, int64_t* launches, double* flops, double* bytes, int n) {
  if (!m || !ms || n < VDR_K_COUNT) return fail(m, VDR_ERR_INVALID, "bad argument");
  for (int k = 0; k < VDR_K_COUNT; ++k) ms[k] = 0.0;
  std::vector<ProfEvent> used;
  used.swap(m->ev_used);  // (an early return below drops the pairs not yet read; none is left behind moved-from)
  for (auto& e : used) {
    VDR_TRY(hipEventSynchronize(e.b.get()), "hipEventSynchronize");
    float t = 0.0f;
    VDR_TRY(hipEventElapsedTime(&t, e.a.get(), e.b.get()), "hipEventElapsedTime");
    ms[e.cls] += t;
    m->ev_free.push_back(std::move(e));
  }
  for (int k = 0; k < VDR_K_COUNT; ++k) {
    if (launches) launches[k] = m->p_launch[k];
    if (flops) flops[k] = m->p_flops[k];
    if (bytes) bytes[k] = m->p_bytes[k];
    m->p_launch[k] = 0;
    m->p_flops[k] = 0;
    m->p_bytes[k] = 0;
  }
  return VDR_OK;
}

}  // extern "C"

// ---- the mask decoder object (include/vdr.h "mask decoder"; kernels: csrc/mask_decoder.hip) -------------------------------------
// The load-time rules of this file hold here too: the device copies live in ONE DevBuf that frees itself with the handle, and a
// name is spelled once -- a checkpoint name in md_names, a derived buffer as a field of MdWeights (both mask_decoder_pack.h).
struct vdr_mask_decoder {
  vdr_mask_decoder_config cfg;
  int device = 0;
  std::vector<MdWeightDef> table;  // md_names: the n_required required weights, then the optional prompt weights
  int n_required = 0;
  int support = 0;  // VDR_PROMPT_POINTS | VDR_PROMPT_MASK: what finalize found complete
  MdHost host;      // what vdr_mask_decoder_set_weight was given
  DevBuf arena;     // what vdr_mask_decoder_finalize built: md_pack's bytes ...
  MdWeights w;      // ... and its fields, pointing into the arena
  bool finalized = false;
};

namespace {

using MD = vdr_mask_decoder;

// the decode's workspace: every buffer 256-byte aligned, in this order
struct MdCarve {
  size_t pe, tok, tmp, qkv, att, q, kv2, h, keys, keys2, img, atti, up, up2, hx1, hx2, hyper, ix1, ix2, total;
};
MdCarve md_carve(const MD* d, int64_t P, int tokens = MD_T) {
  const int64_t n = (int64_t)d->cfg.grid * d->cfg.grid, T = tokens * P;
  MdCarve c{};
  size_t off = 0;
  auto take = [&](int64_t bytes) {
    const size_t o = off;
    off += ((size_t)bytes + 255) / 256 * 256;
    return o;
  };
  c.pe = take(T * MD_C * 2);
  c.tok = take(T * MD_C * 2);
  c.tmp = take(T * MD_C * 2);
  c.qkv = take(T * 3 * MD_C * 2);
  c.att = take(T * MD_C * 2);
  c.q = take(T * MD_IN * 2);
  c.kv2 = take(T * 2 * MD_IN * 2);
  c.h = take(T * (int64_t)d->cfg.mlp_dim * 2);
  c.keys = take(P * n * MD_C * 2);
  c.keys2 = take(P * n * MD_C * 2);
  c.img = take(P * n * 3 * MD_IN * 2);
  c.atti = take(P * n * MD_IN * 2);
  c.up = take(P * n * MD_C * 2);
  c.up2 = take(P * n * MD_C * 2);
  c.hx1 = take(4 * P * MD_C * 2);
  c.hx2 = take(4 * P * MD_C * 2);
  c.hyper = take(4 * P * 32 * 4);
  c.ix1 = take(P * MD_C * 2);
  c.ix2 = take(P * MD_C * 2);
  c.total = off;
  return c;
}

int md_ln(const void* x, void* y, const MdNormW& w, int64_t rows, int D, float eps, hipStream_t s) {
  LnArgs a{};
  a.x = x;
  a.in_bf16 = 1;
  a.y = y;
  a.out_bf16 = 1;
  a.gamma = w.g;
  a.beta = w.b;
  a.rows = rows;
  a.D = D;
  a.eps = eps;
  a.imap = identity_map();
  a.omap = identity_map();
  OP_TRY(launch_layernorm(a, s), "layernorm");
  return VDR_OK;
}

int md_gemm(const void* x, const MdLinW& w, const void* resid, void* y, int64_t M, int N, int K, hipStream_t s) {
  const int epi = resid ? EPI_BIAS_RESID : EPI_BIAS;
  GemmArgs g = linear(x, w.w, y, M, N, K, epi);
  g.bias = w.b;
  g.resid = resid;
  return op_gemm(g, epi, gemm_variant_for(VDR_K_GEMM_FC1, M, N), (void*)s, "mask decoder gemm: unsupported shape");
}

}  // namespace

extern "C" {

int vdr_mask_decoder_create(const vdr_mask_decoder_config* cfg, int device, vdr_mask_decoder_handle* out) {
  const char* op = "vdr_mask_decoder_create";
  if (!cfg || !out) return refuse(op, VDR_ERR_INVALID, "null argument");
  *out = nullptr;
  if (device < 0) return refuse(op, VDR_ERR_INVALID, "device must be >= 0");
  if (cfg->grid < 1 || cfg->grid > 64) return refuse(op, VDR_ERR_UNSUPPORTED, "grid must be 1 .. 64");
  if (cfg->img <= 0) return refuse(op, VDR_ERR_INVALID, "img (the input side the boxes are given in) must be positive");
  if (cfg->channels != 256 || cfg->heads != 8 || cfg->depth != 2 || cfg->attention_downsample_rate != 2 || cfg->mask_tokens != 4 ||
      cfg->upscale_channels_1 != 64 || cfg->upscale_channels_2 != 32 || cfg->iou_head_depth != 3)
    return refuse(op, VDR_ERR_UNSUPPORTED, "channels 256, heads 8, depth 2, attention downsample rate 2, 4 mask tokens, upscale channels 64 / 32, IoU head depth 3");
  if (cfg->mlp_dim <= 0 || cfg->mlp_dim % 64 || cfg->mlp_dim > 2048) return refuse(op, VDR_ERR_UNSUPPORTED, "mlp_dim must be a multiple of 64, at most 2048");
  if (!(cfg->ln_eps > 0.0f) || !(cfg->final_ln_eps > 0.0f) || !(cfg->ln2d_eps > 0.0f)) return refuse(op, VDR_ERR_INVALID, "the eps fields must be positive");
  if (int rc = check_device(nullptr)) return rc;
  DeviceGuard dg(device);  // (only to learn that the device exists)
  if (!dg.ok) return refuse(op, VDR_ERR_HIP, "hipSetDevice failed");
  MD* d = new MD();
  d->cfg = *cfg;
  d->device = device;
  d->table = md_names(cfg->mlp_dim);
  for (const MdWeightDef& w : d->table) d->n_required += w.group == MD_REQUIRED;
  *out = d;
  return VDR_OK;
}

void vdr_mask_decoder_destroy(vdr_mask_decoder_handle d) {
  if (!d) return;
  DeviceGuard dg(d->device);
  delete d;  // (the arena frees itself)
}

int vdr_mask_decoder_num_weights(vdr_mask_decoder_handle d) { return d ? d->n_required : 0; }

const char* vdr_mask_decoder_weight_name(vdr_mask_decoder_handle d, int i) {
  return d && i >= 0 && i < d->n_required ? d->table[i].name.c_str() : nullptr;
}

int vdr_mask_decoder_num_prompt_weights(vdr_mask_decoder_handle d) { return d ? (int)d->table.size() - d->n_required : 0; }

const char* vdr_mask_decoder_prompt_weight_name(vdr_mask_decoder_handle d, int i) {
  return i >= 0 && i < vdr_mask_decoder_num_prompt_weights(d) ? d->table[d->n_required + i].name.c_str() : nullptr;
}

int vdr_mask_decoder_prompt_support(vdr_mask_decoder_handle d) { return d && d->finalized ? d->support : 0; }

int vdr_mask_decoder_set_weight(vdr_mask_decoder_handle d, const char* name, const float* host, const int64_t* shape, int ndim) {
  const char* op = "vdr_mask_decoder_set_weight";
  if (!d || !name || !host || !shape || ndim < 1 || ndim > 4) return refuse(op, VDR_ERR_INVALID, "null or malformed argument");
  if (d->finalized) return refuse(op, VDR_ERR_INVALID, "the decoder is finalized");
  for (const MdWeightDef& w : d->table)
    if (w.name == name) {
      int64_t want = 1, got = 1;
      for (int64_t v : w.shape) want *= v;
      for (int k = 0; k < ndim; ++k) got *= shape[k];
      if (got != want) return refuse(op, VDR_ERR_INVALID, std::string(name) + ": element count mismatch");
      d->host[name].assign(host, host + want);
      return VDR_OK;
    }
  return refuse(op, VDR_ERR_UNKNOWN_NAME, std::string("unknown weight ") + name);
}

int vdr_mask_decoder_finalize(vdr_mask_decoder_handle d) {
  const char* op = "vdr_mask_decoder_finalize";
  if (!d) return refuse(op, VDR_ERR_INVALID, "null handle");
  if (d->finalized) return VDR_OK;
  // the required weights, then the optional groups: all of a group or none of it
  int support = 0;
  for (MdGroup grp : {MD_REQUIRED, MD_POINTS, MD_MASK}) {
    size_t have = 0;
    const MdWeightDef* missing = nullptr;  // the group's first
    for (const MdWeightDef& w : d->table)
      if (w.group == grp) {
        if (d->host.count(w.name)) ++have;
        else if (!missing) missing = &w;
      }
    if (grp == MD_REQUIRED && missing) return refuse(op, VDR_ERR_INCOMPLETE, "missing weight " + missing->name);
    if (grp != MD_REQUIRED && !missing) support |= grp == MD_MASK ? VDR_PROMPT_MASK : VDR_PROMPT_POINTS;
    if (grp != MD_REQUIRED && missing && have)
      return refuse(op, VDR_ERR_INCOMPLETE, std::string(grp == MD_MASK ? "the mask prompt's" : "the point prompts'") + " weights are given in part: missing weight " + missing->name);
  }
  DeviceGuard dg(d->device);
  if (!dg.ok) return refuse(op, VDR_ERR_HIP, "hipSetDevice failed");
  // one staging vector, one allocation, one copy; then every field of d->w is pointed at its offset
  const MdPacked pk = md_pack(d->cfg, d->host, support, d->w);
  DevBuf arena;
  OP_TRY(arena.alloc(pk.bytes.size()), "hipMalloc(mask decoder weights)");
  OP_TRY(hipMemcpy(arena.get(), pk.bytes.data(), pk.bytes.size(), hipMemcpyHostToDevice), "hipMemcpy(mask decoder weights)");
  pk.publish(arena.get());
  d->arena = std::move(arena);
  d->support = support;
  d->host.clear();
  d->finalized = true;
  return VDR_OK;
}

int vdr_mask_decoder_workspace_bytes(vdr_mask_decoder_handle d, int problems, size_t* out) {
  const char* op = "vdr_mask_decoder_workspace_bytes";
  if (!d || !out) return refuse(op, VDR_ERR_INVALID, "null argument");
  if (problems <= 0 || problems > 65535) return refuse(op, VDR_ERR_INVALID, "problems must be 1 .. 65535");
  *out = md_carve(d, problems).total;
  return VDR_OK;
}

int vdr_mask_decoder_workspace_bytes_prompts(vdr_mask_decoder_handle d, int problems, int tokens, size_t* out) {
  const char* op = "vdr_mask_decoder_workspace_bytes_prompts";
  if (!out) return refuse(op, VDR_ERR_INVALID, "null argument");
  if (tokens < 6) return refuse(op, VDR_ERR_INVALID, "a decode has at least 6 tokens per problem");
  if (tokens > MD_MAX_T) return refuse(op, VDR_ERR_UNSUPPORTED, "at most " + std::to_string(MD_MAX_T) + " tokens per problem");
  if (!d) return refuse(op, VDR_ERR_INVALID, "null handle");
  if (problems <= 0 || problems > 65535) return refuse(op, VDR_ERR_INVALID, "problems must be 1 .. 65535");
  *out = md_carve(d, problems, tokens).total;
  return VDR_OK;
}

}  // extern "C"

namespace {

// What both decode entry points ask of their common arguments, refused in this order before the device is touched; pr ==
// nullptr: vdr_mask_decode (boxes alone, T = 7)
int md_check(const char* op, const MD* d, const float* emb, int channels_last, const float* boxes, const vdr_mask_prompts* pr, int T, int batch,
             int boxes_per_image, const void* workspace, size_t workspace_bytes, const float* logits, const float* iou) {
  if (!d || !emb || (!pr && !boxes) || !workspace || !logits || !iou) return refuse(op, VDR_ERR_INVALID, "null argument");
  if (channels_last != 0 && channels_last != 1) return refuse(op, VDR_ERR_INVALID, "channels_last must be 0 or 1");
  if (batch <= 0 || boxes_per_image <= 0 || (int64_t)batch * boxes_per_image > 65535)
    return refuse(op, VDR_ERR_INVALID, "batch and boxes_per_image must be positive, at most 65535 problems");
  if (pr) boxes = pr->boxes;
  if (!aligned16({emb, boxes, pr ? pr->points : nullptr, pr ? pr->labels : nullptr, pr ? pr->mask_input : nullptr, workspace, logits, iou}))
    return refuse(op, VDR_ERR_INVALID, "pointers must be 16-byte aligned");
  if (!d->finalized) return refuse(op, VDR_ERR_INCOMPLETE, "vdr_mask_decoder_finalize has not run");
  if (pr && (pr->points || !pr->boxes) && !(d->support & VDR_PROMPT_POINTS))
    return refuse(op, VDR_ERR_UNSUPPORTED, "point prompts (and the padding point of a decode without boxes) need point_embeddings.{0,1} and not_a_point_embed");
  if (pr && pr->mask_input && !(d->support & VDR_PROMPT_MASK)) return refuse(op, VDR_ERR_UNSUPPORTED, "a mask prompt needs the mask_downscaling weights");
  const MdCarve c = md_carve(d, (int64_t)batch * boxes_per_image, T);
  if (int rc = refuse_workspace(op, workspace_bytes, c.total)) return rc;
  return VDR_OK;
}

// the chain of launches both decode entry points run, on the handle's device; pr == nullptr: vdr_mask_decode's own set-up
int md_run(const char* op, MD* d, const float* emb, int channels_last, const float* boxes, const vdr_mask_prompts* pr, int T, int batch,
           int boxes_per_image, void* workspace, float* logits, float* iou, void* stream) {
  const int P = batch * boxes_per_image, g = d->cfg.grid, n = g * g, C = MD_C, F = d->cfg.mlp_dim;
  const MdCarve c = md_carve(d, P, T);
  if (int rc = check_device(nullptr)) return rc;
  DeviceGuard dg(d->device);
  if (!dg.ok) return refuse(op, VDR_ERR_HIP, "hipSetDevice failed");
  const bool pts = pr && (pr->points || !pr->boxes);  // (a decode without boxes carries a padding point)
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const MdWeights& w = d->w;
  void *pe = ws + c.pe, *tok = ws + c.tok, *tmp = ws + c.tmp, *qkv = ws + c.qkv, *att = ws + c.att, *q = ws + c.q, *kv2 = ws + c.kv2, *h = ws + c.h;
  void *keys = ws + c.keys, *keys2 = ws + c.keys2, *img = ws + c.img, *atti = ws + c.atti, *up = ws + c.up, *up2 = ws + c.up2;
  auto bfp = [](void* p, int64_t off) { return (void*)((char*)p + 2 * off); };
#define MD_L(expr, what) OP_TRY(expr, what)
#define MD_R(call)                  \
  do {                              \
    if (int rc = (call)) return rc; \
  } while (0)
  // tokens (also the query pe) and keys
  if (!pr) {
    MD_L(launch_decoder_setup(boxes, w.fixed, w.gauss, w.corner, emb, channels_last, w.no_mask, pe, keys, batch, boxes_per_image, g, (float)d->cfg.img, s),
         "decoder_setup");
  } else {
    MD_L(launch_prompt_tokens(pr->boxes, pr->points, pr->labels, pr->points ? pr->points_per_problem : 0, w.fixed, w.gauss, w.corner,
                              pts ? w.pt_emb : nullptr, pts ? w.nap : nullptr, pe, P, T, (float)d->cfg.img, s), "prompt_tokens");
    if (pr->mask_input)
      MD_L(launch_mask_embed(emb, channels_last, pr->mask_input, pr->mask_per_image, w.mask_w, w.mask_w + MASK_EMBED_SMALL, w.mask_w + MASK_EMBED_SMALL + 16 * MD_C, keys, P,
                             boxes_per_image, g, d->cfg.ln2d_eps, s), "mask_embed");
    else
      MD_L(launch_decoder_keys(emb, channels_last, w.no_mask, keys, batch, boxes_per_image, g, s), "decoder_keys");
  }
  const void* cur = pe;  // the tokens of layer 0 are the initial ones
  auto tl = [&](const void* x, int64_t ldx, const void* xadd, const MdLinW& l, const void* resid, void* y, int f32out, int64_t ldy, int M, int N, int K,
                int groups, int relu, int rpg = 0, int64_t gs = 0) {
    return launch_token_linear(x, ldx, xadd, C, l.w, l.b, resid, C, y, f32out, ldy, M, N, K, groups, relu, s, rpg, gs);
  };
  // token -> image attention with its out-projection, residual and norm; leaves the new tokens in `tok`
  auto t2i = [&](const MdAttnW& a, int ncols, const MdNormW& norm, float eps) -> int {
    MD_L(tl(cur, C, pe, a.q, nullptr, q, 0, MD_IN, T * P, MD_IN, C, 1, 0), "token_linear");
    MD_R(md_gemm(keys, a.img, nullptr, img, (int64_t)P * n, ncols, C, s));
    MD_L(launch_cross_attention(q, MD_IN, nullptr, img, ncols, a.ktab, bfp(img, MD_IN), ncols, att, MD_IN, P, T, n, 8, 16, s), "cross_attention");
    MD_L(tl(att, MD_IN, nullptr, a.o, cur, tmp, 0, C, T * P, C, MD_IN, 1, 0), "token_linear");
    MD_R(md_ln(tmp, tok, norm, (int64_t)T * P, C, eps, s));
    cur = tok;
    return VDR_OK;
  };
  for (int i = 0; i < 2; ++i) {
    const MdBlockW& L = w.l[i];
    MD_L(tl(cur, C, i ? pe : nullptr, L.qk, nullptr, qkv, 0, 3 * C, T * P, 2 * C, C, 1, 0), "token_linear");
    MD_L(tl(cur, C, nullptr, L.v, nullptr, bfp(qkv, 2 * C), 0, 3 * C, T * P, C, C, 1, 0), "token_linear");
    MD_L(launch_cross_attention(qkv, 3 * C, nullptr, bfp(qkv, C), 3 * C, nullptr, bfp(qkv, 2 * C), 3 * C, att, C, P, T, T, 8, 32, s), "cross_attention");
    MD_L(tl(att, C, nullptr, L.o, i ? cur : nullptr, tmp, 0, C, T * P, C, C, 1, 0), "token_linear");
    MD_R(md_ln(tmp, tok, L.n1, (int64_t)T * P, C, d->cfg.ln_eps, s));
    cur = tok;
    MD_R(t2i(L.t2i, 3 * MD_IN, L.n2, d->cfg.ln_eps));
    MD_L(tl(tok, C, nullptr, L.fc1, nullptr, h, 0, F, T * P, F, C, 1, 1), "token_linear");
    MD_L(tl(h, F, nullptr, L.fc2, tok, tmp, 0, C, T * P, C, F, 1, 0), "token_linear");
    MD_R(md_ln(tmp, tok, L.n3, (int64_t)T * P, C, d->cfg.ln_eps, s));
    MD_L(tl(tok, C, pe, L.k2, nullptr, kv2, 0, 2 * MD_IN, T * P, MD_IN, C, 1, 0), "token_linear");
    MD_L(tl(tok, C, nullptr, L.v2, nullptr, bfp(kv2, MD_IN), 0, 2 * MD_IN, T * P, MD_IN, C, 1, 0), "token_linear");
    MD_L(launch_cross_attention(bfp(img, 2 * MD_IN), 3 * MD_IN, L.qtab, kv2, 2 * MD_IN, nullptr, bfp(kv2, MD_IN), 2 * MD_IN, atti, MD_IN, P, n, T, 8, 16, s),
         "cross_attention");
    MD_R(md_gemm(atti, L.o2, keys, keys2, (int64_t)P * n, C, MD_IN, s));
    MD_R(md_ln(keys2, keys, L.n4, (int64_t)P * n, C, d->cfg.ln_eps, s));
  }
  MD_R(t2i(w.f, 2 * MD_IN, w.fn, d->cfg.final_ln_eps));
  // upscaling: the first transposed convolution as a linear, LayerNorm2d over the 64 channels of each of its 4 sub-pixels
  MD_R(md_gemm(keys, w.up1, nullptr, up, (int64_t)P * n, C, C, s));
  MD_R(md_ln(up, up2, w.up_n, (int64_t)P * n * 4, 64, d->cfg.ln2d_eps, s));
  // the hypernetworks on the mask tokens (rows p * 7 + 1 + m of tok), the IoU head on the IoU token (row p * 7)
  void *hx1 = ws + c.hx1, *hx2 = ws + c.hx2, *hyper = ws + c.hyper, *ix1 = ws + c.ix1, *ix2 = ws + c.ix2;
  MD_L(tl(bfp(tok, C), C, nullptr, w.hy[0], nullptr, hx1, 0, C, 4 * P, C, C, 4, 1, 4, (int64_t)T * C), "token_linear");
  MD_L(tl(hx1, C, nullptr, w.hy[1], nullptr, hx2, 0, C, 4 * P, C, C, 4, 1), "token_linear");
  MD_L(tl(hx2, C, nullptr, w.hy[2], nullptr, hyper, 1, 32, 4 * P, 32, C, 4, 0), "token_linear");
  MD_L(tl(tok, (int64_t)T * C, nullptr, w.iou[0], nullptr, ix1, 0, C, P, C, C, 1, 1), "token_linear");
  MD_L(tl(ix1, C, nullptr, w.iou[1], nullptr, ix2, 0, C, P, C, C, 1, 1), "token_linear");
  MD_L(tl(ix2, C, nullptr, w.iou[2], nullptr, iou, 1, 4, P, 4, C, 1, 0), "token_linear");
  MD_L(launch_mask_upscale(up2, w.up2.w, w.up2.b, (const float*)hyper, logits, P, g, 1, s), "mask_upscale");
#undef MD_L
#undef MD_R
  return VDR_OK;
}

// the prompts alone: what can be refused without a handle comes first (tests/test_sam_prompts_cpu.py has no device to make one with)
int md_check_prompts(const char* op, const vdr_mask_prompts* pr, int* tokens) {
  if (!pr) return refuse(op, VDR_ERR_INVALID, "null prompts");
  if (!pr->boxes && !pr->points) return refuse(op, VDR_ERR_INVALID, "at least one of boxes and points must be given");
  if (pr->points && (!pr->labels || pr->points_per_problem <= 0))
    return refuse(op, VDR_ERR_INVALID, "points need labels and a positive points_per_problem");
  if (pr->mask_per_image != 0 && pr->mask_per_image != 1) return refuse(op, VDR_ERR_INVALID, "mask_per_image must be 0 or 1");
  const int64_t T = 5 + (pr->points ? (int64_t)pr->points_per_problem : 0) + (pr->boxes ? 2 : 1);
  if (T > MD_MAX_T)
    return refuse(op, VDR_ERR_UNSUPPORTED, "at most " + std::to_string(MD_MAX_T) + " tokens per problem (5 + points + 2 with a box, + 1 without); got " + std::to_string(T));
  *tokens = (int)T;
  return VDR_OK;
}

}  // namespace

extern "C" {

int vdr_mask_decode(vdr_mask_decoder_handle d, const float* emb, int channels_last, const float* boxes, int batch, int boxes_per_image,
                    void* workspace, size_t workspace_bytes, float* logits, float* iou, void* stream) {
  const char* op = "vdr_mask_decode";
  if (int rc = md_check(op, d, emb, channels_last, boxes, nullptr, MD_T, batch, boxes_per_image, workspace, workspace_bytes, logits, iou)) return rc;
  return md_run(op, d, emb, channels_last, boxes, nullptr, MD_T, batch, boxes_per_image, workspace, logits, iou, stream);
}

int vdr_mask_decode_prompts(vdr_mask_decoder_handle d, const float* emb, int channels_last, const vdr_mask_prompts* prompts, int batch,
                            int boxes_per_image, void* workspace, size_t workspace_bytes, float* logits, float* iou, void* stream) {
  const char* op = "vdr_mask_decode_prompts";
  int T = 0;
  if (int rc = md_check_prompts(op, prompts, &T)) return rc;
  if (int rc = md_check(op, d, emb, channels_last, nullptr, prompts, T, batch, boxes_per_image, workspace, workspace_bytes, logits, iou)) return rc;
  return md_run(op, d, emb, channels_last, nullptr, prompts, T, batch, boxes_per_image, workspace, logits, iou, stream);
}

}  // extern "C"

