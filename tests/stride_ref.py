"""Pure-torch fp32 restatement of a ViT whose patch convolution runs at a stride below its kernel (TEST HELPER;
vdr_set_patch_stride, "Deep ViT Features as Dense Visual Descriptors"):

    F.conv2d(images, W, b, stride=s) -> flatten(2).transpose(1, 2)                     [B, gh*gw, D]
    pos_embed's patch rows resampled in float64 to (gh, gw), bicubic, align_corners=False, size=, rounded once
    oracle.vit_oracle.assemble_tokens / encoder, unchanged

gh x gw = ((H - p) / s + 1) x ((W - p) / s + 1).  Register tokens (vit_oracle knows none) are inserted after the CLS row
without a position, as tests/dinov3_ref.py's assemble does.  emulate=True rounds pixels and patch weights to bf16 as
vit_oracle.patch_embed(emulate=True) does and hands `emulate` on to the encoder.
"""
import torch
import torch.nn.functional as F

from oracle import vit_oracle as vo


def grid(size, p, s):
    """(gh, gw) of Conv2d(kernel=p, stride=s) over size = (H, W)"""
    H, W = size
    assert H >= p and W >= p and (H - p) % s == 0 and (W - p) % s == 0, (size, p, s)
    return (H - p) // s + 1, (W - p) // s + 1


def interp_pos(pos, g, ncls):
    """pos_embed [1, ncls + g0*g0, D] -> [1, ncls + gh*gw, D]: the CLS row copied, the patch rows resampled in float64
    (tests/test_input_size_gpu.py's _interp64) and rounded to fp32 once; the native grid returns the table itself"""
    D = pos.shape[-1]
    n0 = pos.shape[1] - ncls
    g0 = int(round(n0 ** 0.5))
    assert g0 * g0 == n0, pos.shape
    if tuple(g) == (g0, g0):
        return pos
    t = pos[0, ncls:].double().reshape(1, g0, g0, D).permute(0, 3, 1, 2)
    t = F.interpolate(t, size=tuple(g), mode="bicubic", align_corners=False)
    rows = t.permute(0, 2, 3, 1).reshape(1, g[0] * g[1], D).float()
    return torch.cat([pos[:, :ncls], rows], dim=1)


def patch_embed(images, weight, bias, s, emulate=False):
    """[B, C, H, W] -> [B, gh*gw, D]"""
    return F.conv2d(vo._r(images, bool(emulate)), vo._r(weight, bool(emulate)), bias, stride=s).flatten(2).transpose(1, 2).contiguous()


@torch.no_grad()
def forward_images(cfg: vo.VitCfg, w, images, stride, emulate_bf16=False, registers=None):
    """vit_oracle.forward_images at patch stride `stride`: dict(patch_embed [B, n, D], tokens [B, N, D], cls, dense, grid).
    registers: [1, R, D] register tokens or None."""
    images = images.to(torch.float32)
    g = grid(images.shape[-2:], cfg.patch, stride)
    ncls = 1 if cfg.has_cls else 0
    pe = patch_embed(images, w["patch_embed.proj.weight"], w["patch_embed.proj.bias"], stride, emulate_bf16)
    ws = dict(w)
    if cfg.has_pos:
        ws["pos_embed"] = interp_pos(w["pos_embed"], g, ncls)
    x = vo.assemble_tokens(cfg, ws, pe)
    P = ncls
    if registers is not None:
        R = registers.shape[1]
        x = torch.cat([x[:, :ncls], registers.reshape(1, R, -1).expand(x.shape[0], -1, -1), x[:, ncls:]], dim=1)
        P += R
    if cfg.input_ln:
        x = vo.layer_norm(x, w["input_norm.weight"], w["input_norm.bias"], cfg.ln_eps)
    x = vo.encoder(cfg, w, x, emulate_bf16)
    return {"patch_embed": pe, "tokens": x, "cls": x[:, 0, :].contiguous(), "dense": x[:, P:, :].contiguous(), "grid": g}
