// Host side of the mask decoder object (vdr_api.hip "the mask decoder object"): the one table of its weight names, the typed
// device weights md_run reads, and md_pack, which derives every device buffer from the loaded weights into ONE staging vector.
// No HIP include: tests/mask_decoder_pack_cases.cpp runs all of it on the host.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/vdr.h"

namespace vdr {

inline uint16_t f32_to_bf16(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // keep NaN a NaN
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);                  // round to nearest even
}

constexpr int MD_C = 256, MD_T = 7, MD_IN = 128, MD_MAX_T = 16;

// ---- the weight table: the only place a checkpoint name of the decoder is declared --------------------------------------------
// The ORDER is observable: the MD_REQUIRED entries come first and are vdr_mask_decoder_weight_name's enumeration, the optional
// ones follow (the point prompts' group, then the mask prompt's) and are vdr_mask_decoder_prompt_weight_name's.
enum MdGroup { MD_REQUIRED, MD_POINTS, MD_MASK };
struct MdWeightDef {
  std::string name;
  std::vector<int64_t> shape;
  MdGroup group;
};

inline std::vector<MdWeightDef> md_names(int64_t mlp_dim) {
  std::vector<MdWeightDef> t;
  MdGroup group = MD_REQUIRED;
  auto add = [&](const std::string& n, std::vector<int64_t> shp) { t.push_back({n, std::move(shp), group}); };
  const int64_t C = MD_C, F = mlp_dim;
  auto attn = [&](const std::string& p, int64_t inner) {
    for (const char* n : {"q_proj", "k_proj", "v_proj"}) {
      add(p + n + ".weight", {inner, C});
      add(p + n + ".bias", {inner});
    }
    add(p + "out_proj.weight", {C, inner});
    add(p + "out_proj.bias", {C});
  };
  auto ln = [&](const std::string& p, int64_t n) {
    add(p + ".weight", {n});
    add(p + ".bias", {n});
  };
  add("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix", {2, C / 2});
  add("prompt_encoder.point_embeddings.2.weight", {1, C});
  add("prompt_encoder.point_embeddings.3.weight", {1, C});
  add("prompt_encoder.no_mask_embed.weight", {1, C});
  add("mask_decoder.iou_token.weight", {1, C});
  add("mask_decoder.mask_tokens.weight", {4, C});
  for (int i = 0; i < 2; ++i) {
    const std::string p = "mask_decoder.transformer.layers." + std::to_string(i) + ".";
    attn(p + "self_attn.", C);
    ln(p + "norm1", C);
    attn(p + "cross_attn_token_to_image.", MD_IN);
    ln(p + "norm2", C);
    add(p + "mlp.lin1.weight", {F, C});
    add(p + "mlp.lin1.bias", {F});
    add(p + "mlp.lin2.weight", {C, F});
    add(p + "mlp.lin2.bias", {C});
    ln(p + "norm3", C);
    ln(p + "norm4", C);
    attn(p + "cross_attn_image_to_token.", MD_IN);
  }
  attn("mask_decoder.transformer.final_attn_token_to_image.", MD_IN);
  ln("mask_decoder.transformer.norm_final_attn", C);
  add("mask_decoder.output_upscaling.0.weight", {C, 64, 2, 2});
  add("mask_decoder.output_upscaling.0.bias", {64});
  ln("mask_decoder.output_upscaling.1", 64);
  add("mask_decoder.output_upscaling.3.weight", {64, 32, 2, 2});
  add("mask_decoder.output_upscaling.3.bias", {32});
  for (int m = 0; m < 4; ++m)
    for (int j = 0; j < 3; ++j) {
      const std::string p = "mask_decoder.output_hypernetworks_mlps." + std::to_string(m) + ".layers." + std::to_string(j);
      add(p + ".weight", {j == 2 ? 32 : C, C});
      add(p + ".bias", {j == 2 ? 32 : C});
    }
  for (int j = 0; j < 3; ++j) {
    const std::string p = "mask_decoder.iou_prediction_head.layers." + std::to_string(j);
    add(p + ".weight", {j == 2 ? 4 : C, C});
    add(p + ".bias", {j == 2 ? 4 : C});
  }
  group = MD_POINTS;
  add("prompt_encoder.point_embeddings.0.weight", {1, C});
  add("prompt_encoder.point_embeddings.1.weight", {1, C});
  add("prompt_encoder.not_a_point_embed.weight", {1, C});
  group = MD_MASK;  // (mask_in_chans = 16)
  const std::string m = "prompt_encoder.mask_downscaling.";
  add(m + "0.weight", {4, 1, 2, 2});
  add(m + "0.bias", {4});
  add(m + "1.weight", {4});
  add(m + "1.bias", {4});
  add(m + "3.weight", {16, 4, 2, 2});
  add(m + "3.bias", {16});
  add(m + "4.weight", {16});
  add(m + "4.bias", {16});
  add(m + "6.weight", {C, 16, 1, 1});
  add(m + "6.bias", {C});
  return t;
}
static_assert(4 * 4 + 3 * 4 + 16 * 16 + 3 * 16 + MD_C * 16 + MD_C == VDR_MASK_EMBED_WEIGHTS, "the mask group, packed, is vdr_op_mask_embed's `weights`");

// ---- the device weights a decode reads: bf16 matrices through const void*, fp32 vectors and tables through const float* ------
// (pointers only, every one published by md_pack; a buffer that does not exist is a field that does not exist)
struct MdLinW {
  const void* w = nullptr;
  const float* b = nullptr;
};
struct MdNormW {
  const float *g = nullptr, *b = nullptr;
};
// token -> image attention, of a block and the final one.  img: the image side in one GEMM, columns [k | v] and, in a block,
// [| q of image-to-token]; its bias is v's alone (zeros elsewhere: ktab carries k's with the positional encoding)
struct MdAttnW {
  MdLinW q, o, img;
  const float* ktab = nullptr;  // [n, 128]: pe Wk^T + bk
};
struct MdBlockW {
  MdLinW qk, v, o;  // self-attention (q and k stacked)
  MdAttnW t2i;
  MdLinW fc1, fc2;
  const float* qtab = nullptr;  // [n, 128]: pe Wq^T + bq of image-to-token
  MdLinW k2, v2, o2;            // image -> token
  MdNormW n1, n2, n3, n4;
};
struct MdWeights {
  const float *gauss = nullptr, *corner = nullptr, *fixed = nullptr, *no_mask = nullptr;
  MdBlockW l[2];
  MdAttnW f;
  MdNormW fn;
  MdLinW up1, up2;  // the transposed convolutions as [(dy, dx, Cout), Cin]; up1's bias repeated per sub-pixel
  MdNormW up_n;
  MdLinW hy[3], iou[3];  // (hy: the four hypernetworks stacked)
  // null unless the group was given (vdr_mask_decoder_prompt_support)
  const float *pt_emb = nullptr, *nap = nullptr;
  const float* mask_w = nullptr;  // vdr_op_mask_embed's `weights`
};

// ---- packing ------------------------------------------------------------------------------------------------------------------
using MdHost = std::map<std::string, std::vector<float>>;  // what vdr_mask_decoder_set_weight was given, by name

struct MdSlot {
  const float** dst_f;  // the field of the MdWeights this buffer is published to (one of the two, by the field's type)
  const void** dst_v;
  size_t off, bytes;    // its extent in MdPacked::bytes
};
struct MdPacked {
  std::vector<unsigned char> bytes;  // every buffer at a 256-byte aligned offset
  std::vector<MdSlot> slots;
  // base: where `bytes` was copied to
  void publish(const void* base) const {
    for (const MdSlot& s : slots) {
      const char* p = (const char*)base + s.off;
      if (s.dst_f) *s.dst_f = (const float*)p;
      else *s.dst_v = p;
    }
  }
};

// Everything a decode reads, derived from the loaded weights: bf16 rounding, stacked projections, the float64 positional
// tables at cfg.grid, the permuted transposed convolutions.  `host` holds every MD_REQUIRED weight and all of each group in
// `support` (VDR_PROMPT_POINTS | VDR_PROMPT_MASK), each with the element count of its MdWeightDef.  The slots point into `w`.
inline MdPacked md_pack(const vdr_mask_decoder_config& cfg, const MdHost& host, int support, MdWeights& w) {
  MdPacked out;
  using Vec = std::vector<float>;
  using Parts = std::vector<const Vec*>;  // concatenated in this order
  auto take = [&](size_t bytes, const float** dst_f, const void** dst_v) {
    const size_t off = (out.bytes.size() + 255) / 256 * 256;
    out.bytes.resize(off + bytes);
    out.slots.push_back({dst_f, dst_v, off, bytes});
    return out.bytes.data() + off;
  };
  auto count = [](const Parts& parts) {
    size_t n = 0;
    for (const Vec* p : parts) n += p->size();
    return n;
  };
  auto f32 = [&](const float*& dst, const Parts& parts) {
    unsigned char* o = take(count(parts) * 4, &dst, nullptr);
    for (const Vec* p : parts)
      if (!p->empty()) std::memcpy(o, p->data(), p->size() * 4), o += p->size() * 4;
  };
  auto bf16 = [&](const void*& dst, const Parts& parts) {
    uint16_t* o = reinterpret_cast<uint16_t*>(take(count(parts) * 2, nullptr, &dst));  // (a 256-byte aligned offset of new[]'s bytes)
    for (const Vec* p : parts)
      for (float v : *p) *o++ = f32_to_bf16(v);
  };
  const Vec none;
  auto H = [&](const std::string& name) {
    auto it = host.find(name);
    return it == host.end() ? &none : &it->second;
  };
  auto lin = [&](MdLinW& L, const std::string& p) {
    bf16(L.w, {H(p + ".weight")});
    f32(L.b, {H(p + ".bias")});
  };
  auto norm = [&](MdNormW& N, const std::string& p) {
    f32(N.g, {H(p + ".weight")});
    f32(N.b, {H(p + ".bias")});
  };

  const int g = cfg.grid, n = g * g;
  {  // an upper bound of the arena (every weight as fp32, the five tables, the alignment gaps), so that it never moves
    size_t bound = 5 * (size_t)n * MD_IN * 4 + 128 * 256;
    for (const auto& kv : host) bound += kv.second.size() * 4;
    out.bytes.reserve(bound);
  }
  // the Fourier features of the cell centres, float64: [n, 256]
  const Vec& G = *H("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix");
  std::vector<double> kpe((size_t)n * MD_C);
  for (int y = 0; y < g; ++y)
    for (int x = 0; x < g; ++x)
      for (int f = 0; f < 128; ++f) {
        const double cx = 2.0 * ((x + 0.5) / g) - 1.0, cy = 2.0 * ((y + 0.5) / g) - 1.0;
        const double ph = 6.283185307179586476925286766559 * (cx * (double)G[f] + cy * (double)G[128 + f]);
        kpe[(size_t)(y * g + x) * MD_C + f] = sin(ph);
        kpe[(size_t)(y * g + x) * MD_C + 128 + f] = cos(ph);
      }
  // pe W^T + b on the bf16-rounded weight the GEMM multiplies with: fp32 [n, 128]
  auto table = [&](const float*& dst, const std::string& p) {
    const Vec &W = *H(p + ".weight"), &b = *H(p + ".bias");
    std::vector<double> Wr(W.size());
    for (size_t i = 0; i < W.size(); ++i) {
      const uint32_t u = (uint32_t)f32_to_bf16(W[i]) << 16;
      float r;
      std::memcpy(&r, &u, 4);
      Wr[i] = (double)r;
    }
    Vec t((size_t)n * MD_IN);
    for (int r = 0; r < n; ++r)
      for (int o = 0; o < MD_IN; ++o) {
        double a = 0.0;
        for (int k = 0; k < MD_C; ++k) a += kpe[(size_t)r * MD_C + k] * Wr[(size_t)o * MD_C + k];
        t[(size_t)r * MD_IN + o] = (float)(a + (double)b[o]);
      }
    f32(dst, {&t});
  };
  // ConvTranspose2d weight [Cin, Cout, 2, 2] -> [(dy, dx, Cout), Cin]
  auto convt = [&](const void*& dst, const Vec& W, int Cin, int Cout) {
    Vec o((size_t)4 * Cout * Cin);
    for (int ci = 0; ci < Cin; ++ci)
      for (int co = 0; co < Cout; ++co)
        for (int s = 0; s < 4; ++s) o[((size_t)s * Cout + co) * Cin + ci] = W[((size_t)ci * Cout + co) * 4 + s];
    bf16(dst, {&o});
  };
  const Vec z128(MD_IN, 0.0f);
  // token -> image attention `p`; q_i2t: the block's image-to-token q_proj, the third column group of the image-side GEMM
  auto t2i = [&](MdAttnW& A, const std::string& p, const std::string& q_i2t) {
    lin(A.q, p + "q_proj");
    lin(A.o, p + "out_proj");
    Parts wimg{H(p + "k_proj.weight"), H(p + "v_proj.weight")}, bimg{&z128, H(p + "v_proj.bias")};
    if (!q_i2t.empty()) wimg.push_back(H(q_i2t + ".weight")), bimg.push_back(&z128);
    bf16(A.img.w, wimg);
    f32(A.img.b, bimg);
    table(A.ktab, p + "k_proj");
  };

  f32(w.gauss, {&G});
  f32(w.corner, {H("prompt_encoder.point_embeddings.2.weight"), H("prompt_encoder.point_embeddings.3.weight")});
  f32(w.fixed, {H("mask_decoder.iou_token.weight"), H("mask_decoder.mask_tokens.weight")});
  f32(w.no_mask, {H("prompt_encoder.no_mask_embed.weight")});
  for (int i = 0; i < 2; ++i) {
    MdBlockW& L = w.l[i];
    const std::string p = "mask_decoder.transformer.layers." + std::to_string(i) + ".";
    const std::string s = p + "self_attn.", a = p + "cross_attn_token_to_image.", b = p + "cross_attn_image_to_token.";
    bf16(L.qk.w, {H(s + "q_proj.weight"), H(s + "k_proj.weight")});
    f32(L.qk.b, {H(s + "q_proj.bias"), H(s + "k_proj.bias")});
    lin(L.v, s + "v_proj");
    lin(L.o, s + "out_proj");
    t2i(L.t2i, a, b + "q_proj");
    table(L.qtab, b + "q_proj");
    lin(L.fc1, p + "mlp.lin1");
    lin(L.fc2, p + "mlp.lin2");
    lin(L.k2, b + "k_proj");
    lin(L.v2, b + "v_proj");
    lin(L.o2, b + "out_proj");
    norm(L.n1, p + "norm1");
    norm(L.n2, p + "norm2");
    norm(L.n3, p + "norm3");
    norm(L.n4, p + "norm4");
  }
  t2i(w.f, "mask_decoder.transformer.final_attn_token_to_image.", "");
  norm(w.fn, "mask_decoder.transformer.norm_final_attn");
  {
    const std::string U = "mask_decoder.output_upscaling.";
    convt(w.up1.w, *H(U + "0.weight"), MD_C, 64);
    const Vec* b1 = H(U + "0.bias");
    f32(w.up1.b, {b1, b1, b1, b1});
    norm(w.up_n, U + "1");
    convt(w.up2.w, *H(U + "3.weight"), 64, 32);
    f32(w.up2.b, {H(U + "3.bias")});
  }
  for (int j = 0; j < 3; ++j) {
    Parts hw, hb;
    for (int m = 0; m < 4; ++m) {
      const std::string p = "mask_decoder.output_hypernetworks_mlps." + std::to_string(m) + ".layers." + std::to_string(j);
      hw.push_back(H(p + ".weight"));
      hb.push_back(H(p + ".bias"));
    }
    bf16(w.hy[j].w, hw);
    f32(w.hy[j].b, hb);
    lin(w.iou[j], "mask_decoder.iou_prediction_head.layers." + std::to_string(j));
  }
  if (support & VDR_PROMPT_POINTS) {
    f32(w.pt_emb, {H("prompt_encoder.point_embeddings.0.weight"), H("prompt_encoder.point_embeddings.1.weight")});
    f32(w.nap, {H("prompt_encoder.not_a_point_embed.weight")});
  }
  if (support & VDR_PROMPT_MASK) {  // fp32 on the device: 4.4 K values, in the table's order
    Parts mk;
    for (const MdWeightDef& d : md_names(cfg.mlp_dim))
      if (d.group == MD_MASK) mk.push_back(H(d.name));
    f32(w.mask_w, mk);
  }
  return out;
}

}  // namespace vdr
