// Host program (its own main) over csrc/mask_decoder_pack.h, the host half of the mask decoder object: the weight table, the typed
// device weights and md_pack, which lays every derived buffer out in one arena.  With the staging vector itself as the "device"
// base it checks, for mlp_dim 128 and 2048 at grid 8 and every combination of the two optional groups: that every field of
// MdWeights is published exactly once (the optional ones exactly when their group is given), that the extents are 256-byte
// aligned, pairwise disjoint, inside the arena and as long as the shapes imply, and -- the weights filled with an injective
// function of (name index, element index) -- that the stacked and permuted buffers hold the elements they should.  Built and run
// by tests/test_mask_decoder_pack_cpu.py, once plainly and once with -fsanitize=address,undefined.
#include <cstdio>

#include "mask_decoder_pack.h"

using namespace vdr;

static long long fails = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      if (fails++ < 10) std::printf("FAIL %s (line %d)\n", #cond, __LINE__); \
    }                                                                        \
  } while (0)

// MdWeights is pointers and nothing else, so its fields can be counted as words
constexpr size_t FIELDS = 98;  // 4 + 2 blocks of 32 + 7 + 2 (final attention, its norm) + 4 + 2 (upscaling) + 6 + 6 (heads) + 3 optional
static_assert(sizeof(MdWeights) == FIELDS * sizeof(void*), "a field was added: give it an expected size below");

// element ei of weight ni: distinct floats for distinct (ni, ei), normal and finite; bf16 rounding keeps ni for ei < 2^15
static float fill(size_t ni, size_t ei) {
  const uint32_t u = (uint32_t)((ni + 64) << 20 | ei);
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
static uint16_t bf_at(const void* p, size_t i) {
  uint16_t h;
  std::memcpy(&h, (const unsigned char*)p + 2 * i, 2);
  return h;
}
static uint32_t f32_bits_at(const float* p, size_t i) {
  uint32_t u;
  std::memcpy(&u, (const unsigned char*)p + 4 * i, 4);
  return u;
}
static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

struct Want {
  const void* field;  // address of the field in the MdWeights
  size_t bytes;
};

static void run(int mlp_dim, int support) {
  const int g = 8, n = g * g, C = MD_C, F = mlp_dim;
  vdr_mask_decoder_config cfg{};
  cfg.grid = g;
  cfg.img = 128;
  cfg.mlp_dim = mlp_dim;
  const std::vector<MdWeightDef> table = md_names(mlp_dim);
  MdHost host;
  std::map<std::string, size_t> index;
  size_t n_required = 0, n_points = 0, n_mask = 0;
  for (size_t ni = 0; ni < table.size(); ++ni) {
    const MdWeightDef& d = table[ni];
    CHECK(index.count(d.name) == 0);
    index[d.name] = ni;
    n_required += d.group == MD_REQUIRED;
    n_points += d.group == MD_POINTS;
    n_mask += d.group == MD_MASK;
    if (ni) CHECK(d.group >= table[ni - 1].group);  // required first, then the points' group, then the mask's
    if ((d.group == MD_POINTS && !(support & VDR_PROMPT_POINTS)) || (d.group == MD_MASK && !(support & VDR_PROMPT_MASK))) continue;
    int64_t numel = 1;
    for (int64_t v : d.shape) numel *= v;
    std::vector<float>& h = host[d.name];
    h.resize((size_t)numel);
    for (size_t ei = 0; ei < h.size(); ++ei) h[ei] = fill(ni, ei);
  }
  CHECK(n_points == 3 && n_mask == 10);

  MdWeights w;
  const MdPacked pk = md_pack(cfg, host, support, w);
  const unsigned char* base = pk.bytes.data();
  pk.publish(base);

  // every field once; the optional ones exactly when their group is given
  std::vector<int> published(FIELDS, 0);
  for (const MdSlot& s : pk.slots) {
    CHECK((s.dst_f != nullptr) != (s.dst_v != nullptr));
    const char* dst = s.dst_f ? (const char*)s.dst_f : (const char*)s.dst_v;
    const ptrdiff_t o = dst - (const char*)&w;
    CHECK(o >= 0 && (size_t)o < sizeof(MdWeights) && o % sizeof(void*) == 0);
    if (o >= 0 && (size_t)o < sizeof(MdWeights)) ++published[(size_t)o / sizeof(void*)];
  }
  auto word = [&](const void* field) { return (size_t)((const char*)field - (const char*)&w) / sizeof(void*); };
  for (size_t i = 0; i < FIELDS; ++i) {
    const bool points = i == word(&w.pt_emb) || i == word(&w.nap), mask = i == word(&w.mask_w);
    const bool present = points ? (support & VDR_PROMPT_POINTS) != 0 : mask ? (support & VDR_PROMPT_MASK) != 0 : true;
    CHECK(published[i] == (present ? 1 : 0));
  }
  CHECK((w.pt_emb != nullptr) == ((support & VDR_PROMPT_POINTS) != 0) && (w.nap != nullptr) == (w.pt_emb != nullptr));
  CHECK((w.mask_w != nullptr) == ((support & VDR_PROMPT_MASK) != 0));

  // aligned, inside the arena, pairwise disjoint
  for (size_t i = 0; i < pk.slots.size(); ++i) {
    const MdSlot& a = pk.slots[i];
    CHECK(a.off % 256 == 0 && a.bytes > 0 && a.off + a.bytes <= pk.bytes.size());
    for (size_t j = i + 1; j < pk.slots.size(); ++j) {
      const MdSlot& b = pk.slots[j];
      CHECK(a.off + a.bytes <= b.off || b.off + b.bytes <= a.off);
    }
  }

  // the size of every extent, from the shapes
  std::vector<Want> want;
  auto lin = [&](const MdLinW& l, size_t rows, size_t cols) {
    want.push_back({&l.w, rows * cols * 2});
    want.push_back({&l.b, rows * 4});
  };
  auto norm = [&](const MdNormW& nw, size_t d) {
    want.push_back({&nw.g, d * 4});
    want.push_back({&nw.b, d * 4});
  };
  auto attn = [&](const MdAttnW& a, size_t img_rows) {
    lin(a.q, MD_IN, C);
    lin(a.o, C, MD_IN);
    lin(a.img, img_rows, C);
    want.push_back({&a.ktab, (size_t)n * MD_IN * 4});
  };
  want.push_back({&w.gauss, 2 * 128 * 4});
  want.push_back({&w.corner, 2 * C * 4});
  want.push_back({&w.fixed, 5 * C * 4});
  want.push_back({&w.no_mask, C * 4});
  for (const MdBlockW& L : w.l) {
    lin(L.qk, 2 * C, C);
    lin(L.v, C, C);
    lin(L.o, C, C);
    attn(L.t2i, 3 * MD_IN);
    lin(L.fc1, F, C);
    lin(L.fc2, C, F);
    want.push_back({&L.qtab, (size_t)n * MD_IN * 4});
    lin(L.k2, MD_IN, C);
    lin(L.v2, MD_IN, C);
    lin(L.o2, C, MD_IN);
    for (const MdNormW* nw : {&L.n1, &L.n2, &L.n3, &L.n4}) norm(*nw, C);
  }
  attn(w.f, 2 * MD_IN);
  norm(w.fn, C);
  lin(w.up1, 4 * 64, C);
  lin(w.up2, 4 * 32, 64);
  want.back().bytes = 32 * 4;  // (up2's bias is not repeated: mask_upscale adds it per output channel)
  norm(w.up_n, 64);
  for (int j = 0; j < 3; ++j) {
    lin(w.hy[j], 4 * (j == 2 ? 32 : C), C);
    lin(w.iou[j], j == 2 ? 4 : C, C);
  }
  if (support & VDR_PROMPT_POINTS) {
    want.push_back({&w.pt_emb, 2 * C * 4});
    want.push_back({&w.nap, C * 4});
  }
  if (support & VDR_PROMPT_MASK) want.push_back({&w.mask_w, (size_t)VDR_MASK_EMBED_WEIGHTS * 4});
  CHECK(want.size() == pk.slots.size());
  for (const Want& x : want) {
    int found = 0;
    for (const MdSlot& s : pk.slots)
      if ((s.dst_f ? (const void*)s.dst_f : (const void*)s.dst_v) == x.field) {
        ++found;
        CHECK(s.bytes == x.bytes);
        const void* p = s.dst_f ? (const void*)*s.dst_f : *s.dst_v;
        CHECK(p == base + s.off);
      }
    CHECK(found == 1);
  }

  // the order inside the stacked and permuted buffers
  const std::string l0 = "mask_decoder.transformer.layers.0.", f = "mask_decoder.transformer.final_attn_token_to_image.";
  const size_t sq = index.at(l0 + "self_attn.q_proj.weight"), sk = index.at(l0 + "self_attn.k_proj.weight");
  for (size_t k = 0; k < (size_t)C; ++k) {
    CHECK(bf_at(w.l[0].qk.w, k) == f32_to_bf16(fill(sq, k)));            // row 0: q's row 0
    CHECK(bf_at(w.l[0].qk.w, 256 * C + k) == f32_to_bf16(fill(sk, k)));  // row 256: k's row 0
    CHECK(bf_at(w.l[0].qk.w, 255 * C + k) == f32_to_bf16(fill(sq, 255 * C + k)));
  }
  CHECK(f32_to_bf16(fill(sq, 0)) != f32_to_bf16(fill(sk, 0)));
  const size_t vb0 = index.at(l0 + "cross_attn_token_to_image.v_proj.bias"), vbf = index.at(f + "v_proj.bias");
  for (size_t k = 0; k < (size_t)MD_IN; ++k) {
    CHECK(f32_bits_at(w.l[0].t2i.img.b, k) == 0 && f32_bits_at(w.l[0].t2i.img.b, 2 * MD_IN + k) == 0);
    CHECK(f32_bits_at(w.l[0].t2i.img.b, MD_IN + k) == bits(fill(vb0, k)));
    CHECK(f32_bits_at(w.f.img.b, k) == 0 && f32_bits_at(w.f.img.b, MD_IN + k) == bits(fill(vbf, k)));
  }
  // the image side's third column group is image-to-token's q_proj
  const size_t q2 = index.at(l0 + "cross_attn_image_to_token.q_proj.weight");
  for (size_t k = 0; k < (size_t)C; ++k) CHECK(bf_at(w.l[0].t2i.img.w, 2 * MD_IN * C + k) == f32_to_bf16(fill(q2, k)));
  // ConvTranspose2d [Cin, Cout, 2, 2] -> [(dy, dx, Cout), Cin]
  const size_t u0 = index.at("mask_decoder.output_upscaling.0.weight"), u3 = index.at("mask_decoder.output_upscaling.3.weight");
  for (size_t s = 0; s < 4; ++s)
    for (size_t co = 0; co < 64; ++co)
      for (size_t ci = 0; ci < (size_t)C; ++ci) CHECK(bf_at(w.up1.w, (s * 64 + co) * C + ci) == f32_to_bf16(fill(u0, (ci * 64 + co) * 4 + s)));
  for (size_t s = 0; s < 4; ++s)
    for (size_t co = 0; co < 32; ++co)
      for (size_t ci = 0; ci < 64; ++ci) CHECK(bf_at(w.up2.w, (s * 32 + co) * 64 + ci) == f32_to_bf16(fill(u3, (ci * 32 + co) * 4 + s)));
  const size_t ub = index.at("mask_decoder.output_upscaling.0.bias");
  for (size_t k = 0; k < 256; ++k) CHECK(f32_bits_at(w.up1.b, k) == bits(fill(ub, k % 64)));
  // the four hypernetworks stacked, m-major
  for (size_t m = 0; m < 4; ++m) {
    const size_t hw = index.at("mask_decoder.output_hypernetworks_mlps." + std::to_string(m) + ".layers.2.weight");
    CHECK(bf_at(w.hy[2].w, m * 32 * C + 5) == f32_to_bf16(fill(hw, 5)));
  }
  if (support & VDR_PROMPT_MASK) {  // the mask group in the table's order: 0.weight first, 6.bias last
    CHECK(f32_bits_at(w.mask_w, 0) == bits(fill(index.at("prompt_encoder.mask_downscaling.0.weight"), 0)));
    CHECK(f32_bits_at(w.mask_w, VDR_MASK_EMBED_WEIGHTS - 1) == bits(fill(index.at("prompt_encoder.mask_downscaling.6.bias"), C - 1)));
  }
  std::printf("mlp_dim %d support %d: weights %zu + %zu + %zu, fields %zu, arena %zu bytes\n", mlp_dim, support, n_required, n_points, n_mask,
              pk.slots.size(), pk.bytes.size());
}

int main() {
  int cases = 0;
  for (int mlp_dim : {128, 2048})
    for (int support : {0, VDR_PROMPT_POINTS, VDR_PROMPT_MASK, VDR_PROMPT_POINTS | VDR_PROMPT_MASK}) {
      run(mlp_dim, support);
      ++cases;
    }
  std::printf("cases %d fails %lld\n", cases, fails);
  return fails ? 1 : 0;
}
