"""Records what the descriptor ops of libvdr.so refuse, before a device is touched: tests/golden/descriptor_refusals.json.

    python tests/golden/make_golden_refusals.py path/to/libvdr.so

Run ONCE, against the library built at the commit BEFORE the operand checks of csrc/vdr_api.hip were made one function
(DESIGN.md §4.6q); tests/test_descriptor_refusals_cpu.py replays the table against the library of the day.

For each of the eleven entry points there is one valid argument list on 16-byte-aligned HOST memory (`baselines`, per dtype
where the op takes one) and a list of mutations, each changing one thing (and whatever must follow it to keep the rest valid,
e.g. ld raised with d).  A row is {op, dtype, mutation, code, message}; pointers are spelled "p", "p+4" (null: None), a NaN
"nan".  EVERY ROW MUST BE A REFUSED CALL, -1 (VDR_ERR_INVALID) or -7 (VDR_ERR_UNSUPPORTED): a call that is not refused would,
with a GPU present, launch a kernel on host pointers.  The generator raises on any other code, so the table cannot hold one."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "vit-deep-radiomics_amd"))

F32, BF16 = 0, 1
P = "p"

# role of an argument: what the generic mutations do with it
PTR, OPT, SIZE, D, LD, STRIDE, DTYPE = "ptr16", "opt16", "size", "d", "ld", "stride", "dtype"


def _op(name, dtypes, args, roles, own):
    return dict(name=name, dtypes=dtypes, args=args, roles=roles, own=own)


def _pca(with_imgs, tail, own):
    a = dict(x=P, in_dtype=None, ld=64, image_stride=640, problems=2)
    r = dict(x=PTR, in_dtype=DTYPE, ld=LD, image_stride=STRIDE, problems=SIZE, t=SIZE, d=D)
    if with_imgs:
        a["imgs"], r["imgs"] = 2, SIZE
    a.update(t=10, d=64)
    for n, v in tail.items():
        a[n] = v
        if v == P:
            r[n] = PTR
    a["stream"] = None
    return a, r, own


BIG3 = dict(problems=2 ** 20, imgs=2 ** 6, t=2 ** 5)  # problems * imgs * t = 2^31
BIG2 = dict(problems=2 ** 20, t=2 ** 11)
K8 = [dict(k=0), dict(k=9)]
KM = [dict(k=0, t=4096), dict(k=1025, t=4096), dict(k=21)]  # (R = 20)
KM_ROLES = dict(x=PTR, ld=LD, image_stride=STRIDE, problem_stride=STRIDE, problems=SIZE, imgs=SIZE, t=SIZE, d=D)

OPS = [
    _op("vdr_op_col_mean", (F32, BF16), *_pca(True, dict(work=P, mean=P), [BIG3, dict(d=2080, ld=2080)])),
    _op("vdr_op_covariance", (F32, BF16), *_pca(True, dict(mean=P, work=P, cov=P), [BIG3, dict(d=2080, ld=2080), dict(imgs=1, t=1)])),
    _op("vdr_op_pca_project", (F32, BF16), *_pca(True, dict(mean=P, comps=P, k=3, scale=1, work=P, proj=P, minmax=P),
                                                 [BIG3, dict(d=2080, ld=2080)] + K8)),
    _op("vdr_op_col_mean_any", (F32, BF16), *_pca(False, dict(work=P, mean=P), [BIG2])),
    _op("vdr_op_gram", (F32, BF16), *_pca(False, dict(mean=P, work=P, gram=P), [BIG2, dict(t=1), dict(t=4097)])),
    _op("vdr_op_pca_back_project", (F32, BF16), *_pca(False, dict(mean=P, u=P, values=P, k=3, work=P, comps=P), [BIG2] + K8)),
    _op("vdr_op_kmeans_assign", (BF16,),
        dict(x=P, ld=64, image_stride=640, problem_stride=1280, problems=2, imgs=2, t=10, d=64, k=3, centroids=P, active=None, work=P,
             labels=P, min_dist=P, inertia=P, changed=P, stream=None),
        dict(KM_ROLES, centroids=PTR, active=OPT, work=PTR, labels=PTR, min_dist=PTR, inertia=PTR, changed=PTR), [BIG3] + KM),
    _op("vdr_op_kmeans_update", (BF16,),
        dict(x=P, ld=64, image_stride=640, problem_stride=1280, problems=2, imgs=2, t=10, d=64, k=3, labels=P, active=None, work=P,
             centroids=P, counts=P, stream=None),
        dict(KM_ROLES, labels=PTR, active=OPT, work=PTR, centroids=PTR, counts=PTR), [BIG3] + KM),
    _op("vdr_op_mahalanobis", (BF16,),
        dict(x=P, ld=64, image_stride=640, problem_stride=1280, problems=2, imgs=2, t=10, d=64, mean=P, mean_stride=64, whiten=P,
             whiten_stride=192, k=3, d2=P, stream=None),
        dict(KM_ROLES, mean=PTR, whiten=PTR),
        [BIG3, dict(d2=None), dict(d2="p+2"), dict(k=0), dict(k=2049), dict(k=0, whiten_stride=0), dict(k=2049, whiten_stride=0),
         dict(mean_stride=60), dict(mean_stride=66), dict(mean_stride=-4), dict(whiten_stride=188), dict(whiten_stride=194),
         dict(whiten_stride=-4)]),
    _op("vdr_op_nn_cosine", (BF16,),
        dict(x=P, ldx=64, x_stride=640, tx=10, y=P, ldy=64, y_stride=768, ty=12, pairs=2, d=64, work=P, row_sim=P, row_idx=P, col_sim=P,
             col_idx=P, stream=None),
        dict(x=PTR, ldx=LD, x_stride=STRIDE, tx=SIZE, y=PTR, ldy=LD, y_stride=STRIDE, ty=SIZE, pairs=SIZE, d=D, work=PTR, row_sim=PTR,
             row_idx=PTR),
        [dict(pairs=2 ** 20, tx=2 ** 11), dict(pairs=2 ** 20, ty=2 ** 11), dict(col_sim=None), dict(col_idx=None), dict(col_sim="p+4"),
         dict(col_idx="p+4")]),
    _op("vdr_op_affinity_bits", (BF16,),
        dict(x=P, ldx=64, x_stride=640, t=10, pairs=2, d=64, tau=0.5, exclude_diag=1, work=P, bits=P, pitch=4, stream=None),
        dict(x=PTR, ldx=LD, x_stride=STRIDE, t=SIZE, pairs=SIZE, d=D, work=PTR, bits=PTR),
        [dict(pairs=2 ** 20, t=2 ** 11, pitch=64), dict(pitch=1), dict(pitch=8), dict(tau="nan")]),
]


def mutations(op, dtype):
    base, roles = op["args"], op["roles"]
    half = 4 if dtype == BF16 else 2  # half a 16-byte chunk, in elements
    lds = [n for n, r in roles.items() if r == LD]
    out = []
    for n, r in roles.items():
        if r in (PTR, OPT):
            out += ([{n: None}] if r == PTR else []) + [{n: "p+4"}]
        elif r == SIZE:
            out += [{n: 0}, {n: -1}]
        elif r == D:
            out += [dict({n: 0}), dict({n: -1})] + [dict({n: v}, **{ld: 128 for ld in lds}) for v in (8, 48)]
        elif r == LD:
            out += [{n: base["d"] - 8}, {n: base["d"] + half}]
        elif r == STRIDE:
            out += [{n: -8}, {n: base[n] + half}]
        elif r == DTYPE:
            out += [{n: 2}]
    return out + op["own"]


def native(v, p):
    if isinstance(v, str):
        return float("nan") if v == "nan" else p + int(v[1:] or 0)
    return v


def call(lib, name, args, p):
    """-> (code, message) of one call; `args` in the table's spelling, `p` a 16-byte-aligned host address"""
    code = getattr(lib, name)(*(native(v, p) for v in args.values()))
    msg = lib.vdr_last_error(None)
    return code, msg.decode() if msg else ""


def aligned(n=4096):
    buf = (C.c_char * (n + 16))()
    return buf, (C.addressof(buf) + 15) & ~15


def main(path):
    from vdr import _lib
    lib = _lib.bind(C.CDLL(path), skip_missing=True)
    keep, p = aligned()
    baselines, rows = {}, []
    for op in OPS:
        for dtype in op["dtypes"]:
            tag = "f32" if dtype == F32 else "bf16"
            base = dict(op["args"])
            if "in_dtype" in base:
                base["in_dtype"] = dtype
            baselines.setdefault(op["name"], {})[tag] = base
            for m in mutations(op, dtype):
                code, msg = call(lib, op["name"], dict(base, **m), p)
                if code not in (-1, -7):
                    raise SystemExit(f"{op['name']} {tag} {m}: code {code}, not a refusal -- this row must not be recorded")
                rows.append(dict(op=op["name"], dtype=tag, mutation=m, code=code, message=msg))
    out = os.path.join(HERE, "descriptor_refusals.json")
    with open(out, "w") as f:
        f.write('{"baselines": ' + json.dumps(baselines) + ',\n "rows": [\n  ' + ",\n  ".join(json.dumps(r) for r in rows) + "\n ]}\n")
    print(f"{len(rows)} rows, {len(set(r['message'] for r in rows))} distinct messages -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main(sys.argv[1])
