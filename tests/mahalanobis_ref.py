"""Float64 restatement of vdr_op_mahalanobis' definition (include/vdr.h) and the entry-wise bound between the restatement and
any fp32 evaluation of it.  For tests/test_mahalanobis_gpu.py, tests/test_anomaly_cpu.py, tests/test_anomaly_gpu.py and
tests/golden/make_golden_anomaly.py.

Definition, for rows X [R, d] (values exactly representable in bf16), an fp32 mean [d] and fp32 whitening rows W [k, d]:
    z = fl32(x - mean), ONE fp32 rounding per channel;  z_hi = bf16_rn(z), z_lo = bf16_rn(z - z_hi) (the subtraction is exact);
    w_hi = bf16_rn(w), w_lo = bf16_rn(w - w_hi);
    y_j = z_hi . w_hi_j + z_hi . w_lo_j + z_lo . w_hi_j  (z_lo . w_lo_j is dropped on purpose);   d2_i = sum_j y_j^2.
Here the splits are the stated fp32 / bf16 roundings (`split`, `centre`) and everything after them is float64 (`y`, `d2`).

The bound (`d2_bound`), with u = 2^-24 and g(n) = n u / (1 - n u), the rigorous constant of an fp32 sum of n terms in ANY order:
  * the products of two bf16 values are exact in fp32; y_j accumulates 3 d of them in fp32.  In any order, by operations no
    worse than correctly rounded additions, that errs by at most g(3 d) A_j, A_j = sum_c (|z_hi w_hi| + |z_hi w_lo| + |z_lo w_hi|);
    doubled for an MFMA adder that truncates instead of rounding (the assumption tests/kmeans_ref.py makes of the hardware):
        |dy_j| <= 2 g(3 d) A_j;
  * the square, one rounding: with y^ = y + dy,  |fl(y^ y^) - y^2| <= (2 |y| + |dy|) |dy| + u (|y| + |dy|)^2 =: e_j;
  * the sum of the k squares (the kernel's zero terms past k add nothing), correctly rounded additions in any order:
        |d d2| <= sum_j e_j + g(k) sum_j (y_j^2 + e_j).
What the splits leave, |z - z_hi - z_lo| <= 2^-17 |z| and the dropped lo.lo product (<= 2^-18 |z w|), is part of the DEFINITION,
not of this bound: it separates d2 from the distance with the fp32 operands (tests/test_anomaly_cpu.py measures it against
scikit-learn)."""
import numpy as np
import torch

U = 2.0 ** -24


def g(n):
    return n * U / (1.0 - n * U)


def _f64(t) -> np.ndarray:
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().to(torch.float64).numpy()
    return np.asarray(t, dtype=np.float64)


def bf16_rn(a: np.ndarray) -> np.ndarray:
    """round-to-nearest-even to bf16 of an array of fp32-representable values, returned as float64"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.to(torch.bfloat16).to(torch.float64).numpy()


def bf16_bits(a: np.ndarray) -> np.ndarray:
    """values exactly representable in bf16 -> their uint16 bit patterns"""
    a32 = np.ascontiguousarray(a, dtype=np.float32)
    bits = (a32.view(np.uint32) >> 16).astype(np.uint16)
    assert (from_bf16_bits(bits) == a32).all()
    return bits


def from_bf16_bits(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << 16).view(np.float32)


def split(a) -> tuple:
    """fp32 values -> (hi, lo) as float64"""
    a = _f64(a)
    assert (a.astype(np.float32) == a).all()
    hi = bf16_rn(a)
    return hi, bf16_rn(a - hi)


def centre(x, mean) -> np.ndarray:
    """z = fl32(x - mean) as float64: x [R, d] bf16-representable, mean [d] fp32"""
    x32 = np.ascontiguousarray(_f64(x), dtype=np.float32)
    assert (bf16_rn(x32) == x32).all(), "x must be representable in bf16"
    return (x32 - np.ascontiguousarray(_f64(mean), dtype=np.float32)[None, :]).astype(np.float64)


def y(x, mean, w) -> np.ndarray:
    """the whitened rows [R, k] in float64"""
    zh, zl = split(centre(x, mean))
    wh, wl = split(w)
    return zh @ wh.T + zh @ wl.T + zl @ wh.T


def d2(x, mean, w) -> np.ndarray:
    """[R] float64"""
    v = y(x, mean, w)
    return (v * v).sum(-1)


def d2_bound(x, mean, w) -> np.ndarray:
    """|d d2| [R] of any fp32 evaluation of the definition (module docstring)"""
    zh, zl = split(centre(x, mean))
    wh, wl = split(w)
    d, k = zh.shape[1], wh.shape[0]
    v = zh @ wh.T + zh @ wl.T + zl @ wh.T
    A = np.abs(zh) @ np.abs(wh).T + np.abs(zh) @ np.abs(wl).T + np.abs(zl) @ np.abs(wh).T
    dy = 2.0 * g(3 * d) * A
    e = (2.0 * np.abs(v) + dy) * dy + U * (np.abs(v) + dy) ** 2
    return e.sum(-1) + g(k) * (v * v + e).sum(-1)


def whiten64(cov, shrinkage=0.0, ridge=0.0, n_components=None):
    """float64 numpy restatement of vdr.anomaly.whitening on a 1 / n covariance [d, d] (sklearn's covariance_ of
    EmpiricalCovariance): -> (W [k, d] rounded once to fp32, as float64; eigenvalues [k] descending)"""
    s = _f64(cov)
    d = s.shape[0]
    s = (1.0 - shrinkage) * s + shrinkage * np.trace(s) / d * np.eye(d) + ridge * np.eye(d)
    vals, vecs = np.linalg.eigh(s)
    vals, vecs = vals[::-1], vecs[:, ::-1]
    k = d if n_components is None else n_components
    w = (vecs[:, :k] / np.sqrt(vals[:k])[None, :]).T
    return w.astype(np.float32).astype(np.float64), vals[:k]


def planted(n, d, cond, seed, n_out=0, out_scale=6.0):
    """A planted-spectrum map: n rows N(mu, Q diag(s) Q^T) with the variances s log-spaced from 1 down to 1 / cond and a
    random rotation Q, rounded to bf16; the last n_out rows are outliers, pushed out_scale standard deviations (sqrt(d)
    Mahalanobis units each) along the small-variance directions.  -> (x [n, d] float32, bf16-representable; is_outlier [n])"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    s = np.logspace(0.0, -np.log10(cond), d)
    mu = rng.standard_normal(d) * 0.5
    zz = rng.standard_normal((n, d))
    out = np.zeros(n, bool)
    if n_out:
        out[n - n_out:] = True
        zz[out] += out_scale * np.sign(rng.standard_normal((n_out, d))) * (np.arange(d) >= d // 2)[None, :]
    x = mu[None, :] + (zz * np.sqrt(s)[None, :]) @ q.T
    return bf16_rn(x).astype(np.float32), out
