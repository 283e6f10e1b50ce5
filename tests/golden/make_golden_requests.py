"""Records what the Python front end (vdr/engine.py, vdr/model.py, the refusal half of vdr/pipeline.py) asks of libvdr.so and
of the descriptor ops, without a device: tests/golden/python_requests.json.

    python tests/golden/make_golden_requests.py [--pkg DIR_THAT_HOLDS_vdr] [--out FILE]

Run ONCE, on the commit BEFORE the image, buffer and descriptor plumbing of the two files got one owner each (README_requests.md
names it); tests/test_python_requests_cpu.py imports this file and replays `rows()` against the tree of the day.

Three stubs, none of which touches a device:
  engine rows   an Engine.__new__(Engine) on torch.device("cpu") over a fake library: vdr_workspace_bytes writes through its
                byref argument, every other symbol records its arguments and returns 0.  A row holds the C symbol, every scalar
                argument, every non-pointer struct field, the workspace size, what comes back -- or the exception and the number
                of forward calls the library saw (0).  Pointers are spelled by whose they are: "x" (the caller's images: no
                copy), "ret0".. (the returned tensors), "ws", "other" (a converted copy, the lengths).
  request rows  a VitDescriptorModel.__new__ over such an engine whose forward* methods record their request and stop.
  after rows    the same model with forward_descriptors answering fixed seeded CPU tensors and the vdr.ops / kmeans / spectral /
                anomaly / pca functions the method calls next recording what they are handed (shape, dtype, strides, offset into
                the descriptor buffer: a view, not a copy) and answering fixed tensors."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


class Stop(Exception):
    """raised by the recording engine: the request is on record, nothing runs"""


class FakeLib:
    def __init__(self):
        self.calls = []

    def vdr_workspace_bytes(self, h, batch, seq, ref):
        ref._obj.value = 4096 + 64 * batch + seq
        return 0

    def __getattr__(self, name):
        if not name.startswith("vdr_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def tdesc(t):
    d = {"shape": list(t.shape), "dtype": str(t.dtype)[6:]}
    if not t.is_contiguous():
        d["stride"] = list(t.stride())
    return d


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:12]


def failure(ex, calls):
    return {"raises": type(ex).__name__, "message": str(ex), "calls": calls}


def flat_tensors(ret):
    if isinstance(ret, torch.Tensor):
        return [ret]
    return [t for part in ret for t in flat_tensors(part)]


def make_engine(vdr, cfg, size=None, stride=None):
    e = vdr.engine.Engine.__new__(vdr.engine.Engine)
    e.cfg, e.device, e.h, e._ws, e.lib = cfg, torch.device("cpu"), None, None, FakeLib()
    if size:
        e._size = size
    if stride:
        e._stride = stride
    return e


def engine_call(eng, method, x, *args, owned=(), **kw):
    """one call of an engine entry point -> its row"""
    eng.lib.calls.clear()
    eng._ws = None
    try:
        ret = getattr(eng, method)(x, *args, **kw)
    except Exception as ex:  # noqa: BLE001  (the type is the record)
        return failure(ex, len(eng.lib.calls))
    got = flat_tensors(ret)
    names = {eng._ws.data_ptr(): "ws"}
    for k, t in enumerate(got):
        names.setdefault(t.data_ptr(), f"ret{k}")
    names[x.data_ptr()] = "x"

    def enc(a):
        if isinstance(a, C.Array):
            return [{f: (names.get(getattr(s, f), "other") if f == "out" else getattr(s, f)) for f, _ in s._fields_} for s in a]
        if isinstance(a, int) and not isinstance(a, bool) and a >= 1 << 20:
            return names.get(a, "other")
        return a

    (symbol, cargs), = eng.lib.calls
    return {"symbol": symbol, "args": [enc(a) for a in cargs], "returns": [tdesc(t) for t in got],
            "owned": [[i for i, t in enumerate(got) if t is o] for o in owned]}


def token_cfg(vdr, **kw):
    return vdr.VdrConfig(img=0, patch=0, in_chans=0, dim=64, heads=2, layers=2, mlp_hidden=128, act="gelu", pre_ln=False,
                         has_cls=True, has_pos=False, input_ln=True, ln_eps=1e-5, **kw)


def images(eng, B, dtype=torch.float32):
    h, w = eng.input_size
    return torch.zeros((B, eng.cfg.in_chans, h, w), dtype=dtype)


ENGINES = [("vit_tiny16_224", None, None), ("vit_tiny16_224", (448, 224), None), ("vit_tiny16_224", None, 8),
           ("siglip_base16_224", None, None), ("siglip_base16_224", (448, 224), None), ("siglip_base16_224", None, 8),
           ("dinov3_vits16", None, None), ("medsam", None, None)]


def engine_rows(vdr):
    L = vdr._lib
    LayerOut, AttnMap, FacetOut = vdr.engine.LayerOut, vdr.engine.AttnMap, vdr.engine.FacetOut
    f32, bf16, f16 = torch.float32, torch.bfloat16, torch.float16
    rows = {}

    def put(key, row):
        assert key not in rows, key
        rows[key] = row

    # -- every configuration, batches 1 and 3: one baseline per entry point and per output shape
    for name, size, stride in ENGINES:
        eng = make_engine(vdr, vdr.ARCHS[name], size, stride)
        cfg, sam = eng.cfg, eng.cfg.window > 0
        tag = name + (f"@{size[0]}x{size[1]}" if size else "") + (f"/s{stride}" if stride else "")
        for B in (1, 3):
            x = images(eng, B)
            modes = [L.OUT_ENCODER, L.OUT_PATCH_EMBED] if sam else [L.OUT_CLS, L.OUT_DENSE, L.OUT_PATCH_EMBED, L.OUT_TOKENS]
            for mode in modes:
                put(f"engine/{tag}/B{B}/forward/mode{mode}", engine_call(eng, "forward", x, mode))
                ref = eng.forward(x, mode)
                out = torch.empty(ref.numel(), dtype=bf16)  # (a flat slice of a wider buffer: the element count is what counts)
                put(f"engine/{tag}/B{B}/forward_into/mode{mode}", engine_call(eng, "forward_into", x.to(bf16), out, mode, owned=[out]))
            if sam:
                continue
            D, N, n = cfg.dim, eng.n_tokens, eng.n_patches
            wide = torch.empty((B, 3 * D), dtype=f32)
            specs = [LayerOut(0, L.OUT_CLS, out=wide[:, D:2 * D]), LayerOut(1, L.OUT_POOLED, f32, False), LayerOut(2, L.OUT_DENSE, bf16),
                     LayerOut(cfg.layers - 1, L.OUT_TOKENS)]
            put(f"engine/{tag}/B{B}/forward_layers", engine_call(eng, "forward_layers", x, specs, owned=[specs[0].out]))
            maps = [AttnMap(0, 1), AttnMap(cfg.layers - 1, N, True, bf16)]
            put(f"engine/{tag}/B{B}/forward_attn_maps", engine_call(eng, "forward_attn_maps", x, maps, [LayerOut(1, L.OUT_DENSE)]))
            facets = [FacetOut(cfg.layers - 1), FacetOut(0, "token", 0, True, bf16), FacetOut(1, "value", 2, False, bf16)]
            put(f"engine/{tag}/B{B}/forward_descriptors", engine_call(eng, "forward_descriptors", x, facets, [LayerOut(0)],
                                                                     [AttnMap(cfg.layers - 1, 1, True)]))
            put(f"engine/{tag}/B{B}/forward/wrong_size", engine_call(eng, "forward", torch.zeros(B, 3, x.shape[2] + 16, x.shape[3])))

    # -- vit_tiny16_224, batch 3: every variant an entry point accepts, one at a time ...
    eng = make_engine(vdr, vdr.ARCHS["vit_tiny16_224"])
    cfg, B = eng.cfg, 3
    D, N, n = cfg.dim, eng.n_tokens, eng.n_patches
    x = images(eng, B)

    def ok(key, method, *a, **kw):
        row = engine_call(eng, method, *a, **kw)
        assert "symbol" in row, (key, row)
        put(f"engine/tiny/{method}/{key}", row)

    def no(key, method, *a, **kw):
        row = engine_call(eng, method, *a, **kw)
        assert "raises" in row, (key, row)
        put(f"engine/tiny/{method}/refused/{key}", row)

    strided = torch.zeros(B, 3, 224, 448)[..., ::2]
    for key, xx in (("bf16", x.to(bf16)), ("f64", x.double()), ("u8", x.to(torch.uint8)), ("f16", x.to(f16)), ("strided", strided)):
        ok(f"in_{key}", "forward", xx)
        ok(f"in_{key}", "forward_layers", xx, [LayerOut(3)])
        ok(f"in_{key}", "forward_attn_maps", xx, [AttnMap(3)])
        ok(f"in_{key}", "forward_descriptors", xx, [FacetOut(3)])
    ok("out_bf16", "forward", x, L.OUT_DENSE, bf16)
    for mode in (L.OUT_CLS, L.OUT_POOLED, L.OUT_DENSE, L.OUT_TOKENS):
        for dt in (f32, bf16):
            for norm in (True, False):
                ok(f"mode{mode}_{str(dt)[6:]}_norm{int(norm)}", "forward_layers", x, [LayerOut(5, mode, dt, norm)])
        shape = (B, D) if mode in (L.OUT_CLS, L.OUT_POOLED) else (B, n if mode == L.OUT_DENSE else N, D)
        out = torch.empty(shape, dtype=bf16)
        ok(f"mode{mode}_owned", "forward_layers", x, [LayerOut(5, mode, f32, True, out)], owned=[out])
    one = torch.empty((1, 2 * D))
    ok("one_row_of_a_wide_matrix", "forward_layers", x[:1], [LayerOut(0, L.OUT_CLS, out=one[:, D:])], owned=[])
    ok("generator_of_specs", "forward_layers", x, (LayerOut(i) for i in (1, 2)))
    for q in (1, 2, N):
        for hm in (False, True):
            ok(f"q{q}_hm{int(hm)}", "forward_attn_maps", x, [AttnMap(4, q, hm)])
    out = torch.empty((B, cfg.heads, 1, N), dtype=bf16)
    ok("owned", "forward_attn_maps", x, [AttnMap(4, 1, False, f32, out)], owned=[out])
    ok("bf16", "forward_attn_maps", x, [AttnMap(4, 1, dtype=bf16)])
    ok("no_outs", "forward_attn_maps", x, [AttnMap(0), AttnMap(1)])
    for facet in ("token", "query", "key", "value", L.FACET_KEY):
        ok(f"facet_{facet}", "forward_descriptors", x, [FacetOut(7, facet)])
    for h in (1, 2, 3):
        ok(f"hierarchy{h}", "forward_descriptors", x, [FacetOut(7, "key", h, False, bf16)])
    ok("all_rows", "forward_descriptors", x, [FacetOut(7, "token", 0, True)])
    out = torch.empty((B, n, 9 * D), dtype=bf16)
    ok("owned", "forward_descriptors", x, [FacetOut(7, "key", 1, out=out)], owned=[out])
    ok("facets_only", "forward_descriptors", x, [FacetOut(0), FacetOut(11, "query")])
    ok("with_maps", "forward_descriptors", x, [FacetOut(9)], maps=[AttnMap(11, 1, True)])
    ok("with_outs", "forward_descriptors", x, [FacetOut(9)], [LayerOut(11, L.OUT_CLS)])

    # ... and every refusal, one mutation of such a call each
    meta = lambda shape, dt=f32: torch.empty(shape, dtype=dt, device="meta")  # noqa: E731  (a tensor that lives elsewhere)
    for method, rest in (("forward", ()), ("forward_layers", ([LayerOut(0)],)), ("forward_attn_maps", ([AttnMap(0)],)),
                         ("forward_descriptors", ([FacetOut(0)],))):
        no("three_dims", method, x[0], *rest)
        no("one_channel", method, x[:, :1], *rest)
        no("wrong_width", method, torch.zeros(B, 3, 224, 240), *rest)
    no("unknown_mode", "forward", x, 9)
    good = torch.empty((B, D))
    into = lambda key, xx, out, *a: no(key, "forward_into", xx, out, *a)  # noqa: E731
    into("three_dims", x[0], good)
    into("wrong_width", torch.zeros(B, 3, 224, 240), good)
    into("in_f64", x.double(), good)
    into("out_f16", x, good.to(f16))
    into("in_elsewhere", meta(x.shape), good)
    into("out_elsewhere", x, meta((B, D)))
    into("in_strided", strided, good)
    into("out_strided", x, torch.empty((B, 2 * D))[:, :D])
    into("out_too_small", x, torch.empty((B, D - 1)))
    into("out_too_large", x, torch.empty((B, n, D)), L.OUT_CLS)
    into("unknown_mode", x, good, 9)
    no("empty", "forward_layers", x, [])
    no("mode_patch_embed", "forward_layers", x, [LayerOut(0, L.OUT_PATCH_EMBED)])
    no("dtype_f16", "forward_layers", x, [LayerOut(0, dtype=f16)])
    no("out_f16", "forward_layers", x, [LayerOut(0, out=good.to(f16))])
    no("out_elsewhere", "forward_layers", x, [LayerOut(0, out=meta((B, D)))])
    no("out_shape", "forward_layers", x, [LayerOut(0), LayerOut(0, L.OUT_DENSE, out=torch.empty((B, N, D)))])
    no("out_strided_dense", "forward_layers", x, [LayerOut(0, L.OUT_DENSE, out=torch.empty((B, n, 2 * D))[..., :D])])
    no("out_column_stride", "forward_layers", x, [LayerOut(0, out=torch.empty((D, B)).t())])
    no("out_rows_below_D", "forward_layers", x, [LayerOut(0, L.OUT_POOLED, out=torch.empty(B * D).as_strided((B, D), (D // 2, 1)))])
    no("empty", "forward_attn_maps", x, [])
    no("q_rows_0", "forward_attn_maps", x, [AttnMap(0, 0)])
    no("q_rows_above_N", "forward_attn_maps", x, [AttnMap(0), AttnMap(0, N + 1)])
    no("dtype_f16", "forward_attn_maps", x, [AttnMap(0, dtype=f16)])
    no("out_f16", "forward_attn_maps", x, [AttnMap(0, out=torch.empty((B, cfg.heads, 1, N), dtype=f16))])
    no("out_elsewhere", "forward_attn_maps", x, [AttnMap(0, out=meta((B, cfg.heads, 1, N)))])
    no("out_shape", "forward_attn_maps", x, [AttnMap(0, 1, True, out=torch.empty((B, cfg.heads, 1, N)))])
    no("out_strided", "forward_attn_maps", x, [AttnMap(0, 1, True, out=torch.empty((B, 1, 2 * N))[..., :N])])
    no("bad_layer_out", "forward_attn_maps", x, [AttnMap(0)], [LayerOut(0, 9)])
    no("empty", "forward_descriptors", x, [])
    for key, facet in (("keys", "keys"), ("code7", 7), ("true", True), ("none", None)):
        no(f"facet_{key}", "forward_descriptors", x, [FacetOut(0, facet)])
    no("hierarchy_4", "forward_descriptors", x, [FacetOut(0, "key", 4)])
    no("hierarchy_negative", "forward_descriptors", x, [FacetOut(0, "key", -1)])
    no("binned_all_rows", "forward_descriptors", x, [FacetOut(0, "key", 2, True)])
    no("layer_12", "forward_descriptors", x, [FacetOut(0), FacetOut(12)])
    no("layer_negative", "forward_descriptors", x, [FacetOut(-1)])
    no("dtype_f16", "forward_descriptors", x, [FacetOut(0, dtype=f16)])
    no("out_f16", "forward_descriptors", x, [FacetOut(0, out=torch.empty((B, n, D), dtype=f16))])
    no("out_elsewhere", "forward_descriptors", x, [FacetOut(0, out=meta((B, n, D)))])
    no("out_shape", "forward_descriptors", x, [FacetOut(0, "key", 1, out=torch.empty((B, n, D)))])
    no("out_strided", "forward_descriptors", x, [FacetOut(0, out=torch.empty((B, n, 2 * D))[..., :D])])
    no("bad_layer_out", "forward_descriptors", x, [FacetOut(0)], [LayerOut(0, dtype=f16)])
    no("bad_map", "forward_descriptors", x, [FacetOut(0)], [], [AttnMap(0, 0)])
    others = {"sam": vdr.ARCHS["medsam"], "token_model": token_cfg(vdr), "block_less": vdr.ARCHS["dinov2"],
              "post_ln": vdr.VdrConfig(32, 8, 3, 64, 2, 2, 256, pre_ln=False)}
    for key, c in others.items():
        e2 = make_engine(vdr, c)
        put(f"engine/tiny/forward_descriptors/refused/{key}", engine_call(e2, "forward_descriptors", torch.zeros(1, 3, 32, 32), [FacetOut(0)]))

    # -- a token model
    for has_cls in (True, False):
        eng = make_engine(vdr, token_cfg(vdr) if has_cls else vdr.VdrConfig(**{**token_cfg(vdr).__dict__, "has_cls": False}))
        for Bt in (1, 3):
            t = torch.zeros(Bt, 5, 64)
            for mode in (L.OUT_CLS, L.OUT_DENSE, L.OUT_TOKENS):
                put(f"engine/tokens/cls{int(has_cls)}/B{Bt}/mode{mode}", engine_call(eng, "forward_tokens", t, mode))
        t = torch.zeros(3, 5, 64)
        k = f"engine/tokens/cls{int(has_cls)}/"
        put(k + "bf16_out", engine_call(eng, "forward_tokens", t.to(bf16), L.OUT_CLS, bf16))
        put(k + "f64_in", engine_call(eng, "forward_tokens", t.double()))
        put(k + "lengths_list", engine_call(eng, "forward_tokens", t, lengths=[5, 1, 3]))
        put(k + "lengths_tensor", engine_call(eng, "forward_tokens", t, L.OUT_TOKENS, bf16, lengths=torch.tensor([2, 2, 2])))
        for key, a, kw in (("two_dims", t[0], {}), ("wrong_width", torch.zeros(3, 5, 32), {}), ("unknown_mode", t, {"out_mode": 2}),
                           ("lengths_short", t, {"lengths": [5, 1]}), ("lengths_zero", t, {"lengths": [5, 0, 3]}),
                           ("lengths_above_S", t, {"lengths": [5, 6, 3]})):
            row = engine_call(eng, "forward_tokens", a, **kw)
            assert "raises" in row, (key, row)
            put(k + "refused/" + key, row)

    # -- geometry: properties and host refusals of an engine that holds nothing but its configuration
    for name in ("vit_tiny16_224", "siglip_base16_224", "dinov3_vits16", "medsam", "token"):
        for attrs in ({}, {"_size": (448, 224)}, {"_stride": 8}, {"_size": (160, 96), "_stride": 4}):
            e = vdr.engine.Engine.__new__(vdr.engine.Engine)
            e.cfg = token_cfg(vdr) if name == "token" else vdr.ARCHS[name]
            e.__dict__.update(attrs)
            put(f"engine/geometry/{name}/{sorted(attrs)}", {"input_size": list(e.input_size), "patch_stride": e.patch_stride,
                                                            "grid": list(e.grid), "n_patches": e.n_patches, "n_tokens": e.n_tokens})
        for key, call in (("size_448x224", lambda e: e.set_input_size(448, 224)), ("size_230x224", lambda e: e.set_input_size(230, 224)),
                          ("size_0x224", lambda e: e.set_input_size(0, 224)), ("stride_8", lambda e: e.set_patch_stride(8)),
                          ("stride_5", lambda e: e.set_patch_stride(5)), ("stride_32", lambda e: e.set_patch_stride(32))):
            e = make_engine(vdr, token_cfg(vdr) if name == "token" else vdr.ARCHS[name])
            try:
                call(e)
                row = {"calls": [[s] + list(a[1:]) for s, a in e.lib.calls], "input_size": list(e.input_size), "patch_stride": e.patch_stride}
            except Exception as ex:  # noqa: BLE001
                row = failure(ex, len(e.lib.calls))
            put(f"engine/geometry/{name}/{key}", row)
    return rows


# ---- the model over a recording engine ----------------------------------------------------------------------------------

def spec_desc(s):
    d = dict(s.__dict__)
    d["dtype"] = str(d["dtype"])[6:]
    if d.get("out") is not None:
        o = d["out"]
        d["out"] = dict(tdesc(o), offset=o.storage_offset(), stride=list(o.stride()))
    return {"kind": type(s).__name__, **d}


def enc_arg(a):
    if isinstance(a, torch.dtype):
        return str(a)[6:]
    if isinstance(a, (list, tuple)):
        return [spec_desc(s) if hasattr(s, "__dataclass_fields__") else enc_arg(s) for s in a]
    return a


def make_model(vdr, name, dynamic=False, size=None, stride=None, answer=None):
    """answer: None -- every forward records its request and stops; else answer(request) -> what forward_descriptors returns"""
    m = vdr.VitDescriptorModel.__new__(vdr.VitDescriptorModel)
    m.cfg = vdr.ARCHS[name]
    m.model_name, m.dynamic_size, m.sized, m.device, m.head = name, dynamic, False, torch.device("cpu"), None
    eng = m.engine = make_engine(vdr, m.cfg, size, stride)
    m.log = []

    def recorder(method):
        def fn(x, *a, **kw):
            req = {"method": method, "x": list(getattr(x, "shape", ())), "args": [enc_arg(v) for v in a],
                   "kwargs": {k: enc_arg(v) for k, v in kw.items() if len(v)}}
            m.log.append(req)
            if answer is None or method != "forward_descriptors":
                raise Stop()
            return answer(m, x, *a, **kw)
        return fn
    for method in ("forward", "forward_into", "forward_layers", "forward_attn_maps", "forward_descriptors"):
        setattr(eng, method, recorder(method))
    return m


def model_call(m, fn):
    """fn(m) -> {request | refusal}; the library calls in front of it (vdr_set_input_size) are part of the row"""
    m.log.clear()
    m.engine.lib.calls.clear()
    try:
        fn(m)
        raise AssertionError("a stubbed forward must stop the method")
    except Stop:
        row = {"request": m.log[-1]}
        assert len(m.log) == 1
    except Exception as ex:  # noqa: BLE001
        assert not isinstance(ex, AssertionError), ex
        row = failure(ex, len(m.log))
    if m.engine.lib.calls:
        row["library"] = [[s] + list(a[1:]) for s, a in m.engine.lib.calls]
    return row


def model_cases(vdr):
    """name -> (label, callable(model, x)) of every method at its defaults and with one keyword varied"""
    pipeline = vdr.pipeline
    f32, bf16 = torch.float32, torch.bfloat16
    V = {}

    def add(method, label, fn):
        V.setdefault(method, []).append((label, fn))

    def kwargs(method, variants, call=None):
        for kw in variants:
            label = ",".join(f"{k}={v}" for k, v in kw.items()) or "defaults"
            add(method, label, (lambda kw: (lambda m, x: (call or getattr(m, method))(*((m, x) if call else (x,)), **kw)))(kw))

    for method in ("patch_embed", "image_encoder", "get_last_selfattention", "__call__"):
        kwargs(method, [{}])
    kwargs("forward_features", [{}, {"out_dtype": bf16}])
    kwargs("dense_tokens", [{}, {"out_dtype": f32}])
    kwargs("get_intermediate_layers", [{}, {"n": 4}, {"n": [1, 5, 3]}, {"n": 13}, {"n": [12]}, {"n": []}, {"n": [3, 3]}, {"n": True},
                                       {"reshape": True}, {"return_class_token": True}, {"norm": False}, {"n": 2, "return_class_token": True}])
    kwargs("linear_probe_features", [{}, {"n_last_blocks": 1}, {"avgpool": False}, {"n_last_blocks": 13}])
    kwargs("get_attention_maps", [{}, {"layers": 3}, {"layers": [5, 1, 5]}, {"layers": [0, 12]}, {"layers": []}, {"layers": -1},
                                  {"cls_only": False}, {"head_mean": True}, {"reshape": True}, {"cls_only": False, "reshape": True}])
    common = [{}, {"layer": 9}, {"layer": 12}, {"layer": -1}, {"facet": "token"}, {"facet": "query"}, {"facet": "value"},
              {"facet": "keys"}, {"bin": True}, {"bin": True, "hierarchy": 1}, {"bin": True, "hierarchy": 4}, {"bin": True, "hierarchy": 0},
              {"hierarchy": 4}]
    short = [{}, {"layer": 9}, {"layer": 12}, {"facet": "token"}, {"facet": "keys"}, {"bin": True}, {"bin": True, "hierarchy": 4}]
    kwargs("extract_descriptors", common + [{"include_cls": True}, {"reshape": True}, {"include_cls": True, "reshape": True},
                                            {"bin": True, "include_cls": True}])
    kwargs("upsample_descriptors", common + [{"facet": None}, {"facet": None, "layer": 3}, {"facet": None, "bin": True}, {"radius": 4},
                                             {"radius": 0}, {"sigma_spatial": 0.0}, {"sigma_range": float("nan")}, {"box": (0, 0, 32, 32)},
                                             {"box": (0, 0, 225, 10)}, {"box": (5, 5, 5, 9)}, {"out_dtype": f32},
                                             {"out_dtype": torch.float16}])
    add("find_correspondences", "defaults", lambda m, x: m.find_correspondences(x, x))
    for kw in common[1:] + [{"bin": False}, {"keep_descriptors": True}, {"thresh": 0.5}]:
        add("find_correspondences", ",".join(f"{k}={v}" for k, v in kw.items()), (lambda kw: lambda m, x: m.find_correspondences(x, x, **kw))(kw))
    add("find_correspondences", "other_shape", lambda m, x: m.find_correspondences(x, x[..., :-16]))
    add("find_correspondences", "other_batch", lambda m, x: m.find_correspondences(x, x[:1]))
    kwargs("cosegment", short + [{"k": 4}, {"k": 0}, {"k": 1025}, {"k": 2.5}, {"k": True}, {"k": 1000}, {"thresh": 0.1}])
    kwargs("tokencut", short + [{"tau": 0.3}, {"tau": float("nan")}, {"eps": 1e-3}])
    kwargs("lost", short + [{"k": 10}, {"k": 0}, {"k": 1.5}, {"k": True}, {"tau": 0.1}, {"tau": float("nan")}])
    add("fit_anomaly", "defaults", lambda m, x: m.fit_anomaly([x]))
    for kw in short[1:] + [{"per_position": True}, {"n_components": 8}]:
        add("fit_anomaly", ",".join(f"{k}={v}" for k, v in kw.items()), (lambda kw: lambda m, x: m.fit_anomaly([x], **kw))(kw))
    add("fit_anomaly", "generator", lambda m, x: m.fit_anomaly(x[i:i + 1] for i in range(2)))
    add("fit_anomaly", "no_batches", lambda m, x: m.fit_anomaly([]))

    def gaussian(m, d=None, per_position=False, grid=None, t=1):
        d = m.cfg.dim if d is None else d
        return vdr.anomaly.Gaussian(torch.zeros(t, d), torch.zeros(t, 4, d), torch.ones(t, 4, dtype=torch.float64), 10, per_position, grid)

    add("anomaly_map", "defaults", lambda m, x: m.anomaly_map(x, gaussian(m)))
    for kw in short[1:]:
        width = (1 + 8 * kw.get("hierarchy", 2)) if kw.get("bin") else 1
        add("anomaly_map", ",".join(f"{k}={v}" for k, v in kw.items()),
            (lambda kw, width: lambda m, x: m.anomaly_map(x, gaussian(m, m.cfg.dim * width), **kw))(kw, width))
    add("anomaly_map", "not_a_gaussian", lambda m, x: m.anomaly_map(x, object()))
    add("anomaly_map", "other_width", lambda m, x: m.anomaly_map(x, gaussian(m, 64)))
    add("anomaly_map", "per_position", lambda m, x: m.anomaly_map(x, gaussian(m, None, True, tuple(m.engine.grid), m.engine.n_patches)))
    add("anomaly_map", "per_position_other_grid", lambda m, x: m.anomaly_map(x, gaussian(m, None, True, (3, 3), 9)))
    pca = [{}, {"n_components": 1}, {"n_components": 9}, {"n_components": 0}, {"facet": "key"}, {"facet": "token", "layer": 3},
           {"facet": "keys"}, {"layer": 3}, {"facet": "key", "layer": 12}, {"joint": True}, {"remove_bg": True}]
    kwargs("pca_descriptors", pca)
    kwargs("pca_descriptor_maps", pca + [{"bin": True}, {"facet": "key", "bin": True}, {"facet": "key", "bin": True, "solver": "subspace"},
                                         {"facet": "key", "bin": True, "hierarchy": 4, "solver": "subspace"}, {"solver": "subspace"},
                                         {"solver": "svd"}, {"solver": "subspace", "n_components": 8, "joint": True},
                                         {"facet": "key", "bin": True, "hierarchy": 1, "solver": "subspace", "joint": True}])
    kwargs("get_image_features", [{}, {"normalize": True}])
    add("get_image_features", "with_a_head", lambda m, x: (setattr(m, "head", lambda mm, xx: mm.engine.forward(xx, 0, bf16)), m.get_image_features(x)))
    dense = [{}, {"facet": "key"}, {"facet": "token", "layer": 3}, {"facet": "key", "bin": True}, {"facet": "key", "bin": True, "hierarchy": 1},
             {"layer": 3}, {"bin": True}, {"facet": "keys"}, {"facet": "key", "layer": 12}, {"facet": "key", "bin": True, "hierarchy": 4}]
    kwargs("get_dense_descriptor", dense, call=lambda m, x, **kw: vdr.get_dense_descriptor(m, x[0], **kw))
    add("get_dense_descriptor", "raw_gray", lambda m, x: vdr.get_dense_descriptor(m, np.zeros((1, 1, 1), np.float32)))
    kwargs("extract_dense", dense + [{"encoder": False}], call=lambda m, x, **kw: vdr.extract_dense(m, x, **kw))
    gen = [{"facet": "keys"}, {"layer": 12}, {"bin": True, "hierarchy": 4}, {"include_cls": True}, {"upsample": {"radius": 5}},
           {"upsample": {"sigma": 1.0}}, {"upsample": {"sigma_spatial": -1}}, {"facet": "nope", "upsample": {}}, {"upsampling": {}},
           {"facet": "key", "upsample": {}}]
    for d in gen:
        add("generate_features", json.dumps(d, sort_keys=True),
            (lambda d: lambda m, x: pipeline.generate_features(m, None, None, flip="diagonal", descriptor=d))(d))
    return V


MODELS = ["vit_tiny16_224", "siglip_base16_224", "dinov3_vits16", "medsam", "dinov2"]
SHAPE_METHODS = ("upsample_descriptors", "find_correspondences", "cosegment", "tokencut", "lost", "fit_anomaly", "anomaly_map", "pca_descriptors",
                 "pca_descriptor_maps", "extract_descriptors", "extract_dense", "patch_embed", "image_encoder")


def request_rows(vdr):
    rows = {}
    cases = model_cases(vdr)
    for name in MODELS:
        for method, variants in cases.items():
            # every variant on the plain ViT; the other models at the defaults (and whatever variant names no facet)
            for label, fn in variants if name == "vit_tiny16_224" else [v for v in variants if v[0] == "defaults" or "facet=None" in v[0]]:
                m = make_model(vdr, name)
                x = torch.zeros(2, 3, m.cfg.img, m.cfg.img)
                rows[f"model/{name}/{method}/{label}"] = model_call(m, lambda m: fn(m, x))
    for method in SHAPE_METHODS:  # a batch that is no [B, 3, H, W] batch
        fn = cases[method][0][1]
        for name in ("vit_tiny16_224", "medsam"):
            m = make_model(vdr, name)
            rows[f"model/{name}/{method}/three_dims"] = model_call(m, lambda m: fn(m, torch.zeros(3, m.cfg.img, m.cfg.img)))
    # geometry: another size with and without dynamic_size, a size and a stride in force
    for method, variants in cases.items():
        if method in ("generate_features", "get_dense_descriptor"):
            continue
        fn = variants[0][1]
        for key, kw, hw in (("dynamic_other_size", {"dynamic": True}, (160, 96)), ("dynamic_same_size", {"dynamic": True}, (224, 224)),
                            ("static_other_size", {}, (160, 96)), ("sized_and_strided", {"size": (160, 96), "stride": 8}, (160, 96))):
            m = make_model(vdr, "vit_tiny16_224", **kw)
            rows[f"model/vit_tiny16_224/{method}/{key}"] = model_call(m, lambda m: fn(m, torch.zeros(2, 3, *hw)))
    for name in ("vit_tiny16_224", "medsam", "dinov3_vits16"):  # set_input_size / set_patch_stride of the model
        for key, fn in (("set_input_size", lambda m: m.set_input_size(448, 224)), ("set_input_size_bad", lambda m: m.set_input_size(230, 224)),
                        ("set_patch_stride", lambda m: m.set_patch_stride(8)), ("set_patch_stride_bad", lambda m: m.set_patch_stride(5))):
            m = make_model(vdr, name)
            try:
                ret = fn(m)
                row = {"library": [[s] + list(a[1:]) for s, a in m.engine.lib.calls], "returns_self": ret is m, "grid": list(m.grid),
                       "input_size": list(m.input_size), "patch_stride": m.patch_stride}
            except Exception as ex:  # noqa: BLE001
                row = failure(ex, len(m.engine.lib.calls))
            rows[f"model/{name}/{key}"] = row
    return rows


# ---- what follows the request -------------------------------------------------------------------------------------------

def after_rows(vdr):
    from vdr import anomaly, kmeans, ops, pca, spectral
    rows = {}
    gen = torch.Generator().manual_seed(7)
    state = {}

    def answer(m, x, facets, outs=(), maps=()):
        B, n, N, D = x.shape[0], m.engine.n_patches, m.engine.n_tokens, m.cfg.dim
        got = []
        for f in facets:
            shape = (B, n, (1 + 8 * f.hierarchy) * D) if f.hierarchy else (B, N if f.all_rows else n, D)
            got.append(torch.randn(shape, generator=gen).to(f.dtype))
        state["buffer"] = got[0]
        att = [torch.rand((B, mp.q_rows, N) if mp.head_mean else (B, m.cfg.heads, mp.q_rows, N), generator=gen) for mp in maps]
        state["att"] = att
        return got, [], att

    def seen(t):
        """a tensor a stub is handed: its layout, and where in the descriptor buffer it starts (None: not a view of it)"""
        buf = state["buffer"]
        off = (t.data_ptr() - buf.data_ptr()) // buf.element_size()
        inside = t.dtype == buf.dtype and 0 <= off < max(buf.numel(), 1) and t.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
        return dict(tdesc(t), stride=list(t.stride()), buffer_offset=off if inside else None)

    def note(v):
        if isinstance(v, torch.Tensor):
            return seen(v)
        if isinstance(v, torch.dtype):
            return str(v)[6:]
        if isinstance(v, (tuple, list)):
            return [note(i) for i in v]
        return v if isinstance(v, (int, float, str, bool, type(None))) else type(v).__name__

    fixed = {}

    def stub(mod, name, result):
        real = getattr(mod, name)

        def fn(*a, **kw):
            state["handed"].append({"fn": name, "args": [note(v) for v in a], "kwargs": {k: note(v) for k, v in kw.items()}})
            fixed[name] = result(*a, **kw)
            return fixed[name]
        setattr(mod, name, fn)
        return lambda: setattr(mod, name, real)

    def nn(x, y, mutual=True):
        P, tx, ty = x.shape[0], x.shape[1], y.shape[1]
        return (torch.rand(P, tx, generator=gen), torch.randint(0, ty, (P, tx), generator=gen, dtype=torch.int32),
                torch.rand(P, ty, generator=gen), torch.randint(0, tx, (P, ty), generator=gen, dtype=torch.int32))

    def km(x, k=3, **kw):
        P = 1 if kw.get("joint") else x.shape[0]
        R = x.shape[0] * x.shape[1] // P
        return kmeans.KMeans(torch.randint(0, k, (P, R), generator=gen, dtype=torch.int32), torch.zeros(P, k, x.shape[-1]), None, None, None, None)

    class Acc:
        def __init__(self, per_position=False):
            state["handed"].append({"fn": "GaussianAccumulator", "args": [per_position]})
            self.grid = None

        def add(self, x):
            state["handed"].append({"fn": "add", "args": [seen(x)], "grid": note(self.grid)})

        def finish(self, *a):
            state["handed"].append({"fn": "finish", "args": list(a)})
            return "the accumulator's Gaussian"

    undo = [stub(ops, "nn_cosine", nn), stub(ops, "affinity_bits", lambda x, **kw: torch.zeros(x.shape[0], x.shape[1], (x.shape[1] + 31) // 32, dtype=torch.int32)),
            stub(ops, "upsample_guided", lambda f, g, p, s, **kw: torch.zeros(1)), stub(kmeans, "fit", km),
            stub(kmeans, "elbow", lambda x, **kw: km(x, 5, **kw)), stub(kmeans, "vote", lambda lab, sal, k, *a: torch.arange(k) % 2 == 0),
            stub(spectral, "tokencut", lambda *a, **kw: "the cut"), stub(spectral, "lost", lambda *a, **kw: "the box"),
            stub(pca, "_colorize_maps", lambda x, k, *a: torch.rand(x.shape[0], x.shape[1], k, generator=gen)),
            stub(anomaly.Gaussian, "score", lambda self, x: torch.rand(x.shape[0], x.shape[1], generator=gen))]
    real_acc, anomaly.GaussianAccumulator = anomaly.GaussianAccumulator, Acc

    def result(v):
        if isinstance(v, torch.Tensor):
            same = [k for k, f in fixed.items() if f is v]
            return dict(seen(v), digest=digest(v), is_answer_of=same[0] if same else None)
        if hasattr(v, "__dataclass_fields__"):
            return {k: result(getattr(v, k)) for k in v.__dataclass_fields__}
        if isinstance(v, (tuple, list)):
            return [result(i) for i in v]
        return v if isinstance(v, (int, float, str, bool, type(None))) else type(v).__name__

    def run(key, fn, name="vit_tiny16_224", **kw):
        m = make_model(vdr, name, answer=answer, **kw)
        state["handed"] = []
        fixed.clear()
        try:
            ret = fn(m)
            row = {"requests": list(m.log), "handed": state["handed"], "result": result(ret)}
        except Exception as ex:  # noqa: BLE001
            row = failure(ex, len(m.log))
        rows[f"after/{key}"] = row

    try:
        x = torch.zeros(2, 3, 224, 224)
        gauss = lambda d, pp=False, t=1, grid=None: anomaly.Gaussian(torch.zeros(t, d), torch.zeros(t, 4, d), torch.ones(t, 4), 10, pp, grid)  # noqa: E731
        for kw in ({}, {"reshape": True}, {"include_cls": True}, {"bin": True, "reshape": True}, {"layer": 3, "facet": "token"}):
            run(f"extract_descriptors/{kw}", lambda m: m.extract_descriptors(x, **kw))
        for kw in ({}, {"bin": True, "hierarchy": 1}, {"box": (8, 8, 40, 72), "radius": 3, "out_dtype": torch.float32}, {"layer": 2}):
            run(f"upsample_descriptors/{kw}", lambda m: m.upsample_descriptors(x, **kw))
        run("upsample_descriptors/u8_guide", lambda m: m.upsample_descriptors(x.to(torch.uint8)))
        run("upsample_descriptors/strided", lambda m: m.upsample_descriptors(torch.zeros(2, 3, 160, 96)), size=(160, 96), stride=8)
        for kw in ({}, {"bin": False}, {"keep_descriptors": True}, {"thresh": 0.5}, {"layer": 9, "hierarchy": 1}):
            run(f"find_correspondences/{kw}", lambda m: m.find_correspondences(x, x, **kw))
        run("find_correspondences/dinov3", lambda m: m.find_correspondences(x[:1], x[:1]), name="dinov3_vits16")
        run("find_correspondences/dynamic", lambda m: m.find_correspondences(torch.zeros(1, 3, 160, 96), torch.zeros(1, 3, 160, 96)), dynamic=True)
        for kw in ({}, {"k": 4}, {"bin": True}, {"k": 3, "thresh": 0.5, "votes_percentage": 50, "seed": 3}, {"elbow": 0.9, "max_iter": 5},
                   {"k": 393}):
            run(f"cosegment/{kw}", lambda m: m.cosegment(x, **kw))
        run("cosegment/dinov3", lambda m: m.cosegment(x, k=2), name="dinov3_vits16")
        for kw in ({}, {"tau": 0.3, "eps": 1e-3}, {"bin": True, "layer": 5}):
            run(f"tokencut/{kw}", lambda m: m.tokencut(x, **kw))
        for kw in ({}, {"k": 10, "tau": 0.1}, {"facet": "value"}):
            run(f"lost/{kw}", lambda m: m.lost(x, **kw))
        run("lost/strided", lambda m: m.lost(torch.zeros(1, 3, 160, 96)), size=(160, 96), stride=8)
        for kw in ({}, {"per_position": True}, {"shrinkage": 0.1, "ridge": 1e-3, "n_components": 8}, {"bin": True, "hierarchy": 1}):
            run(f"fit_anomaly/{kw}", lambda m: m.fit_anomaly([x, x[:1]], **kw))
        run("fit_anomaly/per_position_other_grid", lambda m: m.fit_anomaly([x, torch.zeros(1, 3, 160, 96)], per_position=True), dynamic=True)
        run("fit_anomaly/global_other_grid", lambda m: m.fit_anomaly([x, torch.zeros(1, 3, 160, 96)]), dynamic=True)
        run("fit_anomaly/second_batch_three_dims", lambda m: m.fit_anomaly([x, x[0]]))
        run("anomaly_map/global", lambda m: m.anomaly_map(x, gauss(192)))
        run("anomaly_map/binned", lambda m: m.anomaly_map(x, gauss(9 * 192), bin=True, hierarchy=1))
        run("anomaly_map/per_position", lambda m: m.anomaly_map(x, gauss(192, True, 196, (14, 14))))
        run("anomaly_map/per_position_no_grid", lambda m: m.anomaly_map(x, gauss(192, True, 196)))
        run("anomaly_map/per_position_other_rows", lambda m: m.anomaly_map(x, gauss(192, True, 195)))
        for kw in ({"facet": "key"}, {"facet": "token", "layer": 3, "n_components": 2, "joint": True, "remove_bg": True},
                   {"facet": "key", "bin": True, "hierarchy": 1, "solver": "subspace"}):
            run(f"pca_descriptor_maps/{kw}", lambda m: m.pca_descriptor_maps(x, **kw))
        run("pca_descriptors/facet", lambda m: m.pca_descriptors(x, facet="value"))
    finally:
        for u in undo:
            u()
        anomaly.GaussianAccumulator = real_acc
    return rows


def rows(vdr):
    """every row of the table, computed on the package `vdr` (already imported)"""
    real = vdr.engine._stream_ptr
    vdr.engine._stream_ptr = lambda device: 0
    try:
        with torch.no_grad():
            return {**engine_rows(vdr), **request_rows(vdr), **after_rows(vdr)}
    finally:
        vdr.engine._stream_ptr = real


def dump(table, path):
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in table.items()) + "\n}\n")


def main(argv):
    pkg = os.path.join(os.path.dirname(os.path.dirname(HERE)), "vit-deep-radiomics_amd")
    out = os.path.join(HERE, "python_requests.json")
    if "--pkg" in argv:
        pkg = argv[argv.index("--pkg") + 1]
    if "--out" in argv:
        out = argv[argv.index("--out") + 1]
    sys.path.insert(0, pkg)
    import vdr
    assert os.path.dirname(os.path.dirname(os.path.abspath(vdr.__file__))) == os.path.abspath(pkg), vdr.__file__
    table = rows(vdr)
    dump(table, out)
    refused = sum("raises" in r for r in table.values())
    print(f"{len(table)} rows ({refused} refusals) from {pkg} -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main(sys.argv[1:])
