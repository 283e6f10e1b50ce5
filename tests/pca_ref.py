"""float64 restatement of the three PCA definitions of include/vdr.h (vdr_op_col_mean, vdr_op_covariance,
vdr_op_pca_project), the entry-wise fp32 summation bounds that go with them, designed-input generators, and the
composition (fit / colorize / Otsu) that the golden files are compared with.  CPU only; torch and numpy.

A problem is a [R, d] matrix of rows (the images of a joint problem concatenated).  The one step of the definitions that is
not float64 here is the one they fix bit for bit: the centring float(x) - mean is a single IEEE fp32 subtraction, and the
covariance rounds that difference once to bf16."""
import numpy as np
import torch

U = 2.0 ** -24  # unit roundoff of fp32


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def f32(a) -> torch.Tensor:
    return torch.as_tensor(a).to(torch.float32)


# ---- the definitions -------------------------------------------------------------------------------------------------
def col_mean(x: torch.Tensor):
    """x [R, d] (bf16 / fp32 values) -> (mean float64 [d], bound float64 [d]): S / R, and what an fp32 sum of the R terms in
    any order followed by one division may differ by."""
    xd = x.double()
    R = x.shape[0]
    mean = xd.sum(0) / R
    bound = gamma(R) * xd.abs().sum(0) / R + U * mean.abs() + 1e-45
    return mean, bound


def centred_bf16(x: torch.Tensor, mean: torch.Tensor) -> torch.Tensor:
    """z = bf16_rn(float(x) - mean): fp32 subtraction, one rounding to bf16; returned as float64"""
    return (f32(x) - f32(mean)).to(torch.bfloat16).double()


def gram(x: torch.Tensor, mean: torch.Tensor) -> torch.Tensor:
    """z^T z, float64 [d, d]"""
    z = centred_bf16(x, mean)
    return z.t() @ z


def covariance(x: torch.Tensor, mean: torch.Tensor):
    """-> (cov float64 [d, d], bound [d, d]): z^T z / (R - 1); the products are exact in fp32, so the error is that of
    summing R terms (any order: gamma_R) and of one division."""
    z = centred_bf16(x, mean)
    R = x.shape[0]
    cov = z.t() @ z / (R - 1)
    bound = gamma(R) * (z.abs().t() @ z.abs()) / (R - 1) + U * cov.abs() + 1e-45
    return cov, bound


def project(x: torch.Tensor, mean: torch.Tensor, comps: torch.Tensor):
    """-> (proj float64 [R, k], bound [R, k]): sum_c fl(float(x) - mean) * comps[j, c]; each product is rounded once and the
    d terms are summed in fp32 in some order: gamma_{d+1}."""
    v = (f32(x) - f32(mean)).double()
    c = f32(comps).double()
    proj = v @ c.t()
    bound = gamma(x.shape[1] + 1) * (v.abs() @ c.abs().t()) + 1e-45
    return proj, bound


def exact_f32_div(s: torch.Tensor, n: int) -> torch.Tensor:
    """fp32(s) / fp32(n) as one IEEE fp32 division (s must be exactly representable)"""
    assert bool((s.double() == s.float().double()).all())
    return s.float() / torch.tensor(float(n), dtype=torch.float32)


# ---- designed inputs ---------------------------------------------------------------------------------------------------
def designed(problems: int, R: int, d: int, seed: int):
    """Integer maps [problems, R, d] in [-4, 4] whose columns are drawn from different distributions (so a column
    permutation or a tile swap shows), and an integer mean [problems, d] in [-2, 2].  Every centred value (|.| <= 6, exact
    in bf16), every product and -- for R <= 2049 -- every partial sum is an integer below 2^24: any fp32 summation order
    gives the same bits."""
    g = torch.Generator().manual_seed(seed)
    kind = torch.arange(d) % 4
    u = torch.randint(-4, 5, (problems, R, d), generator=g)
    pos = torch.randint(0, 5, (problems, R, d), generator=g)
    sparse = torch.randint(-4, 5, (problems, R, d), generator=g) * (torch.rand((problems, R, d), generator=g) < 0.25)
    ramp = ((torch.arange(R).view(1, R, 1) + torch.arange(d).view(1, 1, d) * 3 + torch.arange(problems).view(-1, 1, 1)) % 9) - 4
    x = torch.where(kind == 0, u, torch.where(kind == 1, pos, torch.where(kind == 2, sparse, ramp.expand(problems, R, d))))
    mean = torch.randint(-2, 3, (problems, d), generator=g)
    return x.to(torch.float32), mean.to(torch.float32)


def designed_components(problems: int, k: int, d: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, (problems, k, d), generator=g).to(torch.float32)


# ---- the composition -----------------------------------------------------------------------------------------------------
def fit(x: torch.Tensor, k: int = 3):
    """The library's route on one map, in float64 around the two rounded steps: fp32 mean (rounded from the float64 sum),
    bf16-centred covariance, eigh, top k descending, svd_flip(u_based_decision=False), components rounded to fp32.
    -> (mean fp32 [d], components fp32 [k, d], explained_variance float64 [k], ratio float64 [k])"""
    mean = col_mean(x)[0].float()
    cov = covariance(x, mean)[0].float().double()
    w, v = torch.linalg.eigh(cov)
    lam = w.flip(0)[:k]
    vec = v.flip(1)[:, :k].t()
    a = vec.abs()
    d = x.shape[1]
    first = torch.where(a == a.max(dim=1, keepdim=True).values, torch.arange(d), d).min(dim=1).values
    sign = torch.sign(torch.gather(vec, 1, first.unsqueeze(1)))
    sign = torch.where(sign == 0, torch.ones_like(sign), sign)
    return mean, (vec * sign).float(), lam, lam / torch.diagonal(cov).sum()


def min_max_scale(a):
    lo, hi = a.min(), a.max()
    return (a - lo) / (hi - lo) if hi != lo else a


def otsu(ch: np.ndarray, nbins: int = 256) -> float:
    """skimage 0.18's threshold_otsu on a float map, restated with numpy"""
    ch = np.asarray(ch, dtype=np.float64).ravel()
    if np.all(ch == ch[0]):
        return float(ch[0])
    counts, edges = np.histogram(ch, bins=nbins, range=(ch.min(), ch.max()))
    counts = counts.astype(float)
    centers = (edges[:-1] + edges[1:]) / 2
    w1 = np.cumsum(counts)
    w2 = np.cumsum(counts[::-1])[::-1]
    m1 = np.cumsum(counts * centers) / w1
    m2 = (np.cumsum((counts * centers)[::-1]) / w2[::-1])[::-1]
    var12 = w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2
    return float(centers[np.argmax(var12)])


def colorize(x: torch.Tensor, output_shape, remove_bg: bool = False):
    """the reference's pca_colorize through `fit` -> (rgb float64 numpy, mask bool numpy or None)"""
    mean, comps, _, _ = fit(x, 3)
    rgb = min_max_scale(project(x, mean, comps)[0]).numpy().reshape(tuple(output_shape) + (3,))
    mask = None
    if remove_bg:
        mask = rgb[..., 0] > otsu(rgb[..., 0])
        rgb = min_max_scale(rgb * mask[..., None])
    return rgb, mask


def component_cosine(a, b) -> np.ndarray:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs((a * b).sum(-1)) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


# ---- the golden files and their gates ----------------------------------------------------------------------------------
SK_CASES = ("pca_sk_64x64", "pca_sk_196x768", "pca_sk_1024x256")
# 4 x the worst value this restatement measured against the golden files (tests/golden/README_pca.md has both numbers):
# the summation order differs between builds of torch and between the host and the device.
GATE_COS = 4 * 3.93e-7      # 1 - |cos| of a component                     (measured 3.93e-7, pca_sk_64x64)
GATE_EV = 4 * 4.18e-4       # explained variance, relative                 (measured 4.18e-4, pca_sk_64x64)
GATE_RATIO = 4 * 4.97e-4    # explained variance ratio, relative           (measured 4.97e-4, pca_sk_64x64)
GATE_RGB = 4 * 1.06e-4      # scaled map against sklearn, absolute         (measured 1.06e-4, pca_sk_64x64)
GATE_REF_RGB = 4 * 2.78e-5  # scaled map against the reference's function, with and without remove_bg (measured 2.78e-5)


def load_golden(golden_dir, name):
    """(npz, x): x fp32, or bf16 where the file stores 16-bit patterns"""
    import os
    g = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    if "x" in g:
        return g, torch.from_numpy(g["x"])
    return g, torch.from_numpy((g["x_bf16_bits"].astype(np.uint32) << 16).view(np.float32)).to(torch.bfloat16)
