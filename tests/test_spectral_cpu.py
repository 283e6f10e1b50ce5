"""CPU: vdr.spectral without a device.  fiedler runs with the device product replaced by a torch stand-in (B v with v rounded
to fp32 and an fp32 sum, as the kernel's) on every golden (tests/golden/README_spectral.md) and is held to SciPy's dense
eigen-decomposition; the TokenCut and LOST host rules are checked on hand-made grids against tests/spectral_ref.py.

Gates, from the perturbation the fp32 product is (u = 2^-24): rounding v and summing in fp32 perturbs M = D^-1/2 W D^-1/2 by at
most about 2 u ||M|| = 2 u in norm per application (t u (B |v|) is the worst case; the sums here are of like-signed cluster
blocks, and the ratio is printed), so the eigenvalue moves by <= 2 u to first order and the eigenvector by
sin(angle) <= 2 * 2 u / gap (Davis-Kahan), gap = min(lambda_3 - lambda_2, lambda_2 - lambda_1) of the golden:
    |lambda - golden| <= 4 u                     (doubled for margin)
    1 - |cos|          <= (8 u / gap)^2 / 2 + t 2^-52   (doubled angle; the float64 evaluation of the cosine itself)."""
import numpy as np
import pytest
import torch

import spectral_ref as sref

from spectral_ref import NAMES, labels_agree, load_golden

U32 = 2.0 ** -24


def standin(B: torch.Tensor):
    """the device product's stand-in for the graphs B [P, t, t] bool: v rounded once to fp32, an fp32 sum"""
    Bf = B.to(torch.float32)
    return lambda bits, v: torch.matmul(Bf, v.to(torch.float32).unsqueeze(-1))[..., 0].to(torch.float64)


@pytest.mark.parametrize("name", NAMES)
def test_golden_files_are_what_the_generator_states(name):
    g, t, b, x = load_golden(name)
    assert np.array_equal(sref.graph(x[None], float(g["tau"]))[0], b)
    assert np.array_equal(b, b.T) and b.diagonal().all()
    s = sref.similarity(x[None])
    margin = np.abs(s - float(np.float32(0.2))) / sref.bound(x[None], s)
    margin[0][np.arange(t), np.arange(t)] = np.inf
    assert margin.min() > 4.0
    vals, vec = sref.fiedler_dense(b, float(g["eps"]), 4)
    assert np.allclose(vals, g["eigvals"], rtol=0, atol=1e-12) and abs(vals[0]) < 1e-12
    assert 1.0 - abs(float(vec @ g["fiedler"])) < 1e-12
    part, seed, mask, box = sref.tokencut(g["fiedler"], tuple(g["grid"]))
    assert np.array_equal(part, g["bipartition"]) and seed == int(g["seed"]) and np.array_equal(mask, g["mask"])
    assert tuple(box) == tuple(g["box"]) and mask.reshape(-1)[seed] and not (mask & ~part).any()


@pytest.mark.parametrize("name", NAMES)
def test_fiedler_with_a_stand_in_product_matches_scipy(name):
    from vdr import ops, spectral
    g, t, b, _ = load_golden(name)
    B = torch.from_numpy(b)[None]
    bits = ops.pack_bits(B)
    vec, val, resid, steps = spectral.fiedler(bits, eps=float(g["eps"]), product=standin(B))
    assert vec.dtype == torch.float64 and tuple(vec.shape) == (1, t) and tuple(val.shape) == (1,) and 1 <= steps <= 32
    lam = g["eigvals"]
    gap = min(lam[2] - lam[1], lam[1] - lam[0])
    dl = abs(float(val[0]) - lam[1])
    dc = 1.0 - abs(float(vec[0].numpy() @ g["fiedler"]))
    print(f"{name}: steps {steps}, |lambda - golden| {dl:.3e} (gate {4 * U32:.3e}), 1 - |cos| {dc:.3e} "
          f"(gate {(8 * U32 / gap) ** 2 / 2 + t * 2.0 ** -52:.3e}), residual estimate {float(resid[0]):.3e}")
    assert float(resid[0]) <= 1e-6
    assert dl <= 4 * U32
    assert dc <= (8 * U32 / gap) ** 2 / 2 + t * 2.0 ** -52
    assert abs(float(vec[0].norm()) - 1.0) < 1e-12 and float(vec[0][vec[0].abs().argmax()]) > 0
    labels_agree(vec[0].numpy(), g, name)
    again = spectral.fiedler(bits, eps=float(g["eps"]), product=standin(B))
    assert torch.equal(again[0], vec) and torch.equal(again[1], val)  # the seeded start: the same from run to run


def test_fiedler_runs_problems_in_lockstep_and_survives_a_disconnected_graph():
    from vdr import ops, spectral
    g, t, b, _ = load_golden("130x32")
    two = np.zeros((t, t), bool)  # two cliques without an edge between them: only eps connects W
    two[:50, :50] = True
    two[50:, 50:] = True
    ring = np.eye(t, dtype=bool)  # a ring: slow convergence, the full 32 steps
    i = np.arange(t)
    ring[i, (i + 1) % t] = ring[(i + 1) % t, i] = True
    B = torch.from_numpy(np.stack([b, two, ring]))
    bits = ops.pack_bits(B)
    vec, val, resid, steps = spectral.fiedler(bits, product=standin(B))
    assert torch.isfinite(vec).all() and torch.isfinite(val).all() and steps == 32
    # problem 0 is the golden, whatever runs next to it
    assert abs(float(val[0]) - g["eigvals"][1]) <= 4 * U32
    labels_agree(vec[0].numpy(), g, "lockstep")
    # the cliques: lambda_2 is of the order of eps, the vector has one sign per clique
    want, wvec = sref.fiedler_dense(two, 1e-5, 3)
    assert abs(float(val[1]) - want[1]) <= 4 * U32 and want[1] < 1e-4
    v = vec[1].numpy()
    assert (np.sign(v[:50]) == np.sign(v[0])).all() and (np.sign(v[50:]) == -np.sign(v[0])).all()
    assert 1.0 - abs(float(v @ wvec)) < 1e-9
    one = spectral.fiedler(bits[1:2], product=standin(B[1:2]))
    assert abs(float(one[1][0]) - want[1]) <= 4 * U32  # alone it stops at the first check; both runs are within the gate
    with pytest.raises(ValueError):
        spectral.fiedler(bits[:, :1, :])
    with pytest.raises(ValueError):
        spectral.fiedler(bits, eps=0.0)


def test_seed_component_and_box_against_scipy():
    from vdr import spectral
    rng = np.random.default_rng(0)
    for gh, gw in ((1, 1), (1, 7), (5, 4), (9, 11)):
        for _ in range(6):
            m = rng.random((gh, gw)) < 0.6
            for seed in rng.integers(0, gh * gw, 4):
                got = spectral.seed_component(m, int(seed))
                assert np.array_equal(got, sref.component(m, int(seed))), (gh, gw, seed)
                if got.any():
                    assert spectral.mask_box(got) == sref.box(got)
    # 4-connectivity: a diagonal neighbour is not connected
    m = np.array([[1, 0], [0, 1]], bool)
    assert spectral.seed_component(m, 0).sum() == 1


def test_tokencut_rule_flips_to_the_seed_and_keeps_its_component():
    from vdr import ops, spectral
    # a 4 x 5 grid: the large-magnitude entries are NEGATIVE, so v > mean misses the seed and the partition must flip
    v = np.full((4, 5), 0.1)
    v[1:3, 1:3] = -0.9
    v[1, 1] = -1.0       # the seed
    v[3, 4] = -0.8       # same side, not connected to the seed's block
    part, seed = spectral.bipartition_rule(v.reshape(-1))
    assert seed == 6 and part.reshape(4, 5)[1, 1] and part.sum() == 5 and part.reshape(4, 5)[3, 4]
    rp, rs, rm, rb = sref.tokencut(v, (4, 5))
    assert rs == seed and np.array_equal(rp.reshape(-1), part)
    assert rm.sum() == 4 and not rm[3, 4] and rb == (1, 1, 2, 2)
    assert np.array_equal(spectral.seed_component(part.reshape(4, 5), seed), rm)
    # ties in |v|: the lowest index is the seed; positive seed: no flip
    v2 = np.array([0.5, -0.5, 0.5, 0.0])
    part2, seed2 = spectral.bipartition_rule(v2)
    assert seed2 == 0 and part2.tolist() == [True, False, True, False]
    # end to end with the stand-in product, P = 2: the assembled result against the reference rules on its own eigenvector
    g, t, b, _ = load_golden("130x32")
    B = torch.from_numpy(np.stack([b, b[::-1, ::-1].copy()]))
    res = spectral.tokencut(ops.pack_bits(B), (10, 13), stride=8, patch=16, product=standin(B))
    assert isinstance(res, spectral.TokenCut) and tuple(res.eigvec.shape) == (2, 10, 13) and res.grid == (10, 13)
    assert 1 <= res.steps <= 32 and tuple(res.bits.shape) == (2, 130, 8) and tuple(res.resid.shape) == (2,)
    for p in range(2):
        rp, rs, rm, rb = sref.tokencut(res.eigvec[p].numpy(), (10, 13))
        assert np.array_equal(res.bipartition[p].numpy(), rp) and int(res.seed[p]) == rs
        assert np.array_equal(res.mask[p].numpy(), rm) and tuple(res.box[p].tolist()) == rb
    assert torch.equal(res.pixel_box(), res.box.float() * 8 + 8.0)
    assert abs(float(res.eigval[0]) - g["eigvals"][1]) <= 4 * U32
    with pytest.raises(ValueError):
        spectral.tokencut(ops.pack_bits(B), (10, 12), product=standin(B))


def test_lost_rule_seed_ties_and_expansion_set():
    from vdr import spectral
    # a 3 x 4 grid, 12 patches: an "object" of 4 patches {0, 1, 4, 11} that see each other only, background sees background
    t, obj = 12, [0, 1, 4, 11]
    b = np.zeros((t, t), bool)
    bg = [i for i in range(t) if i not in obj]
    b[np.ix_(obj, obj)] = True
    b[np.ix_(bg, bg)] = True
    deg = b.sum(1)
    assert set(deg[obj]) == {4} and set(deg[bg]) == {8}
    seed, chosen = spectral.lost_rule(lambda s: b[s], deg, k=6)
    assert seed == 0  # four patches tie on the lowest degree: the lowest index
    # the 6 lowest-degree patches are the object and, by index, background 2 and 3: not adjacent to the seed
    assert sorted(np.nonzero(chosen)[0].tolist()) == obj
    rs, rset, rm, rb = sref.lost(b, (3, 4), 6)
    assert rs == seed and np.array_equal(rset.reshape(-1), chosen)
    # the seed's 4-connected component of the set: 0, 1, 4 touch; 11 is the far corner
    assert sorted(np.nonzero(rm.reshape(-1))[0].tolist()) == [0, 1, 4] and rb == (0, 0, 1, 1)
    assert np.array_equal(spectral.seed_component(chosen.reshape(3, 4), seed), rm)
    # k = 2: only the two lowest (degree, index) patches may join
    _, c2 = spectral.lost_rule(lambda s: b[s], deg, k=2)
    assert sorted(np.nonzero(c2)[0].tolist()) == [0, 1]
    # a seed that is not its own neighbour (exclude_diag graphs) still belongs to its set
    b2 = b & ~np.eye(t, dtype=bool)
    s3, c3 = spectral.lost_rule(lambda s: b2[s], b2.sum(1), k=1)
    assert s3 == 0 and c3[0] and c3.sum() == 1


def test_public_names():
    import vdr
    assert vdr.TokenCut is vdr.spectral.TokenCut and vdr.Lost is vdr.spectral.Lost
    for name in ("tokencut", "lost"):
        assert callable(getattr(vdr.VitDescriptorModel, name))
    for name in ("affinity_bits", "bits_matvec", "unpack_bits", "pack_bits", "bits_pitch"):
        assert callable(getattr(vdr.ops, name))
