"""Float64 restatement of vdr_op_affinity_bits' definition (include/vdr.h), the entry-wise bound between it and any fp32
evaluation, the bit packing, a dense float64 Fiedler solver and the TokenCut / LOST rules, for tests/test_affinity_cpu.py,
tests/test_spectral_cpu.py, tests/test_affinity_gpu.py, tests/test_spectral_model_gpu.py and
tests/golden/make_golden_spectral.py.

Definition, for X [t, d] (values exactly representable in bf16):
    ss(v) = sum_c v_c^2,  rn(v) = 1 / max(sqrt(ss(v)), 1e-8),  sim(i, j) = dot(x_i, x_j) * (rn(x_i) * rn(x_j))
    B[i, j] = sim(i, j) > tau, the diagonal cleared with exclude_diag.
Here every step is float64 (`similarity`, `graph`).

The bound (`bound`) is nn_cosine_ref.bound's derivation with the two norms multiplied first; u = 2^-24, s the float64
similarity, A_ij = sum_c |x_ic x_jc| * rn_i * rn_j:
  * dot: products of two bf16 values are exact in fp32; an fp32 sum of d exact terms in any order errs by at most
    (d - 1) u sum|x y| to first order.  Scaled by the norms: d u A_ij.
  * rn: ss is such a sum of d non-negative terms, relative error <= d u, halved by the square root; sqrtf and the division
    are correctly rounded, u each.  Per norm (d / 2 + 2) u, both (d + 4) u |s|.
  * the product of the two norms: u |s|; the product of dot with it: u |s|.  (nn_cosine: two multiplications by a norm -- the
    same count, so the same bound.)
  Sum: d u (A + |s|) + 6 u |s| <= d u (A + |s|) + 8 u |s| (second-order terms); bound = 2 * that, doubled for margin.
An entry of B may differ from the float64 graph only where |s - tau| <= bound + the rounding of tau itself to fp32.

Packing: bit (j & 31) of word [i, j >> 5] is B[i, j]; rows are pitch = 4 ceil(t / 128) int32 words; everything else 0.

Fiedler pair: W = eps + (1 - eps) B, D = diag(W 1), scipy.linalg.eigh(D - W, D), ascending: value 1, vector 1."""
import os

import numpy as np
import torch

import nn_cosine_ref as nr

U = nr.U
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("130x32", "333x96", "520x416")


def similarity(x) -> np.ndarray:
    """x [P, t, d] (any float dtype) -> float64 sim [P, t, t], in the definition's association"""
    x = nr._f64(x)
    rn = nr.rnorm(x)
    return np.einsum("pic,pjc->pij", x, x) * (rn[:, :, None] * rn[:, None, :])


def graph(x, tau: float, exclude_diag: bool = False) -> np.ndarray:
    """bool [P, t, t]: sim > float32(tau) (the op's threshold is an fp32 value)"""
    b = similarity(x) > float(np.float32(tau))
    if exclude_diag:
        i = np.arange(b.shape[1])
        b[:, i, i] = False
    return b


def bound(x, s: np.ndarray) -> np.ndarray:
    return nr.bound(x, x, s)


def random_maps(P: int, t: int, d: int, seed: int) -> torch.Tensor:
    """bf16 [P, t, d]: unit Gaussian noise plus a_i times one shared unit-scale direction per problem, a_i uniform in [0, 2):
    the scores a_i a_j / sqrt((1 + a_i^2)(1 + a_j^2)) + noise spread over [0, 0.8], so a band of the bound's width around
    tau = 0.2 holds few entries at any d while both kinds of entries are plentiful"""
    gen = torch.Generator().manual_seed(seed)
    noise = torch.randn(P, t, d, generator=gen)
    shared = torch.randn(P, 1, d, generator=gen)
    a = 2.0 * torch.rand(P, t, 1, generator=gen)
    return (noise + a * shared).to(torch.bfloat16)


def band_share(s: np.ndarray, bnd: np.ndarray, tau: float) -> float:
    """share of the entries of s within the bound of float32(tau)"""
    return float((np.abs(s - float(np.float32(tau))) <= bnd).mean())


def pitch(t: int) -> int:
    return (t + 127) // 128 * 4


def pack(b: np.ndarray) -> np.ndarray:
    """bool [P, t, t] -> int32 [P, t, pitch(t)]"""
    P, t, _ = b.shape
    full = np.zeros((P, t, pitch(t) * 32), np.uint64)
    full[:, :, :t] = b
    words = (full.reshape(P, t, -1, 32) << np.arange(32, dtype=np.uint64)).sum(-1)
    return words.astype(np.uint32).view(np.int32)


def unpack(bits: np.ndarray, t: int) -> np.ndarray:
    """int32 [P, t, pitch] -> bool [P, t, t]; the padding bits must be 0"""
    w = np.ascontiguousarray(bits).view(np.uint32).astype(np.uint64)
    full = ((w[..., None] >> np.arange(32, dtype=np.uint64)) & 1).reshape(bits.shape[0], bits.shape[1], -1).astype(bool)
    assert not full[:, :, t:].any(), "padding bits set"
    return full[:, :, :t]


def fiedler_dense(b: np.ndarray, eps: float = 1e-5, k: int = 4):
    """b [t, t] bool -> (the k smallest generalised eigenvalues of (D - W) y = lambda D y ascending, the eigenvector of the
    second one scaled to unit Euclidean norm)"""
    import scipy.linalg
    W = eps + (1.0 - eps) * b.astype(np.float64)
    D = np.diag(W.sum(1))
    vals, vecs = scipy.linalg.eigh(D - W, D)
    v = vecs[:, 1]
    return vals[:k], v / np.linalg.norm(v)


def component(mask: np.ndarray, seed: int) -> np.ndarray:
    """the 4-connected component of mask [gh, gw] that holds the flat index seed (scipy.ndimage.label's default structure)"""
    import scipy.ndimage
    lab, _ = scipy.ndimage.label(mask)
    l = lab.reshape(-1)[seed]
    return (lab == l) & (l > 0)


def box(mask: np.ndarray):
    ys, xs = np.nonzero(mask)
    return int(ys.min()), int(xs.min()), int(ys.max()), int(xs.max())


def tokencut(eigvec: np.ndarray, grid):
    """TokenCut's rule: (bipartition [gh, gw], seed, mask [gh, gw], box).  seed = argmax |v| (first on a tie); bipartition =
    v > mean(v), complemented when it misses the seed; mask its 4-connected component holding the seed."""
    v = np.asarray(eigvec, np.float64).reshape(-1)
    seed = int(np.abs(v).argmax())
    part = v > v.mean()
    if not part[seed]:
        part = ~part
    part = part.reshape(grid)
    m = component(part, seed)
    return part, seed, m, box(m)


def lost(b: np.ndarray, grid, k: int):
    """LOST's rule on the graph b [t, t] (tau = 0): (seed, set [gh, gw], mask, box).  seed: the lowest degree, the lowest index
    on a tie; set: the seed and those of the k lowest-degree patches (ties by index) adjacent to it."""
    deg = b.sum(1)
    order = sorted(range(len(deg)), key=lambda i: (deg[i], i))
    seed = order[0]
    s = np.zeros(len(deg), bool)
    for i in order[:k]:
        s[i] = bool(b[seed, i])
    s[seed] = True
    s = s.reshape(grid)
    m = component(s, seed)
    return seed, s, m, box(m)


def planted(t: int, d: int, seed: int, tau: float = 0.2):
    """The golden maps: three planted clusters with overlapping centres.  c = three unit-normalised Gaussian draws, then
    c1 += 0.35 c0, c2 += 0.15 (c0 + c1); row i = centre[i % 3] + 0.9 * noise / sqrt(d), rounded to bf16; any row with an
    off-diagonal score within 4 x bound of tau is redrawn until none is left.  Returns (x [t, d] fp32 holding bf16 values,
    entries inside the band on the first draw, redraw rounds)."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((3, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    c[1] += 0.35 * c[0]
    c[2] += 0.15 * (c[0] + c[1])

    def draw(rows):
        raw = c[rows % 3] + 0.9 * rng.standard_normal((len(rows), d)) / np.sqrt(d)
        return torch.from_numpy(raw).to(torch.bfloat16).to(torch.float32).numpy()

    x = draw(np.arange(t))
    first, rounds = None, 0
    while True:
        s = similarity(x[None])
        near = np.abs(s - float(np.float32(tau))) <= 4.0 * bound(x[None], s)
        near[0][np.arange(t), np.arange(t)] = False
        if first is None:
            first = int(near.sum())
        bad = np.nonzero(near[0].any(1))[0]
        if bad.size == 0:
            return x, first, rounds
        x[bad] = draw(bad)
        rounds += 1


def load_golden(name):
    g = np.load(os.path.join(GOLDEN, f"spectral_sp_{name}.npz"))
    t = g["fiedler"].shape[0]
    b = np.unpackbits(g["graph"], axis=1)[:, :t].astype(bool)
    x = torch.from_numpy(g["x_bf16"]).view(torch.bfloat16)
    return g, t, b, x


def labels_agree(vec, g, what):
    """the bipartition of vec against the golden's, leaving out rows with |f_i - mean| <= 1e-3 max|f - mean| of the golden
    vector (at most 2 % of the rows; none on the three committed maps)"""
    f = g["fiedler"]
    dev = np.abs(f - f.mean())
    keep = dev > 1e-3 * dev.max()
    assert keep.mean() >= 0.98, what
    v = np.asarray(vec, np.float64).reshape(-1)
    part = v > v.mean()
    want = g["bipartition"].reshape(-1)
    # (each rule flips to its own seed: equal up to the complement)
    same = np.array_equal(part[keep], want[keep]) or np.array_equal(~part[keep], want[keep])
    assert same, what
