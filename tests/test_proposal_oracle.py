"""The NumPy model of the proposal (tests/proposal_oracle.py) anchored independently of the engine: Philox4x32-10 against the
Random123 known answers, the normals against the standard normal, the pdf against scipy on every covariance the GPU tests
feed, the LAPACK route's own deviation from the constructed eigen-systems (the yardstick of tests/test_gpu_proposal.py)."""
import numpy as np
import pytest

from oracle import rbpf_oracle as orc
from tests import proposal_oracle as po

CASES = po.covariance_cases()

# Random123's kat_vectors for philox4x32 with 10 rounds: counter, key, output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr, key, want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert tuple(po.philox4x32_10(ctr, key)) == want
    got = po.philox4x32_10([np.array([c, c], dtype=np.uint64) for c in ctr], [np.uint64(k) for k in key])   # the array form
    assert [g.tolist() for g in got] == [[w, w] for w in want]


def test_u01_is_53_bits_in_the_half_open_unit_interval():
    assert po.u01(0, 0) == 2.0 ** -53 and po.u01(0xffffffff, 0xffffffff) == 1.0
    assert po.u01(0, 1 << 11) == 2.0 ** -52 and po.u01(1, 0) == (2.0 ** 21 + 1) * 2.0 ** -53
    assert po.u01(0, (1 << 11) - 1) == 2.0 ** -53                                    # the low 11 bits of the second word are dropped
    a, b = np.array([0, 0xffffffff, 1], dtype=np.uint64), np.array([0, 0xffffffff, 0], dtype=np.uint64)
    assert po.u01(a, b).tolist() == [po.u01(0, 0), 1.0, po.u01(1, 0)]


def test_normals3_scalar_and_array_forms_agree_and_depend_on_every_argument():
    seed = 2 ** 63 + 5
    base = po.normals3(seed, 3, 1000, 7)
    arr = po.normals3(seed, 3, np.array([1000, 2 ** 31 + 9 - 2 ** 32]), np.array([7, 7]))   # an int32 id above 2^31 wraps to its 32 bits
    assert np.array_equal(arr[0], base) and np.array_equal(arr[1], po.normals3(seed, 3, 2 ** 31 + 9, 7))
    for other in [(seed + 1, 3, 1000, 7), (seed ^ (1 << 40), 3, 1000, 7), (seed, 4, 1000, 7), (seed, 3, 1001, 7), (seed, 3, 1000, 8)]:
        assert not np.any(po.normals3(*other) == base)


def test_normals3_are_standard_normal_and_uncorrelated():
    """10^5 draws of (z0, z1, z2): every mean within 4 sigma (4 / sqrt(N)), every variance within 4 sqrt(2 / N) of 1, every
    pairwise covariance within 4 / sqrt(N) of 0, fourth moments within 4 sqrt(96 / N) of 3 (Var z^4 = 96)."""
    N = 100_000
    gid, k = np.divmod(np.arange(N), 32)
    z = po.normals3(42, 1, gid, k)
    assert z.shape == (N, 3) and np.all(np.isfinite(z))
    assert np.all(np.abs(z.mean(axis=0)) < 4 / np.sqrt(N))
    c = (z.T @ z) / N
    assert np.all(np.abs(np.diag(c) - 1) < 4 * np.sqrt(2 / N))
    assert np.all(np.abs(c[np.triu_indices(3, 1)]) < 4 / np.sqrt(N))
    assert np.all(np.abs((z ** 4).mean(axis=0) - 3) < 4 * np.sqrt(96 / N))
    # z0, z1 share a radius: independent all the same (their squares are uncorrelated: Cov(z0^2, z1^2) = 0, sd 2 / sqrt(N))
    assert abs(np.mean(z[:, 0] ** 2 * z[:, 1] ** 2) - 1) < 4 * np.sqrt(8 / N)


@pytest.mark.parametrize("name, truth", CASES, ids=[n for n, _ in CASES])
def test_model_pdf_is_scipys(name, truth):
    """pdf10 on the LAPACK frame = scipy.stats.multivariate_normal.pdf(allow_singular=True) * 10 = the project's mvn_pdf * 10.
    mvn_pdf runs the same eigh: same operations up to their order, 1e-12 relative (|log c| + maha <= 60, a few ulp in the
    exponent).  scipy runs another LAPACK driver: two backward-stable eigen-solvers differ by some ulp of lam_max in every
    eigenvalue, lam_max / lam_min,kept times that relative in 1 / lam_min, so the log of the pdf moves by up to
    (1 + maha) / 2 times the frame floor 64 * 2^-53 * lam_max / lam_min,kept (1.1e-8 measured at kappa = 1e9, bound 7e-6).
    scipy 1.15 also returns 0 for a point off the support of a singular covariance (residual along the dropped
    eigenvectors >= eps), which neither mvn_pdf nor the filter does: the samples here are drawn inside the support.  For the
    zero matrix eps is 0 and scipy's test `residual < eps` rejects the mean itself: that case is compared with mvn_pdf only."""
    from scipy.stats import multivariate_normal
    rng = np.random.Generator(np.random.PCG64(5))
    mean = np.array([0.3, -0.2, 0.1])
    f = po.frame_from_cov(truth.cov)
    g = mean + rng.standard_normal((40, 3)) @ (f.A * np.any(f.U != 0, axis=0)).T     # the kept directions only
    got = po.pdf10(g, mean, f.U, f.log_c)
    maha = np.sum(((g - mean) @ f.U) ** 2, axis=-1)
    if truth.rank > 0:
        want = multivariate_normal.pdf(g, mean, truth.cov, allow_singular=True) * 10
        assert np.all(want > 0)
        np.testing.assert_allclose(got, want, rtol=1e-12 + po.frame_floor(truth) * (1 + float(maha.max())) / 2)
    np.testing.assert_allclose(got, orc.mvn_pdf(g, mean, truth.cov) * 10, rtol=1e-12)
    assert f.rank == multivariate_normal(mean, truth.cov, allow_singular=True).cov_object.rank == truth.rank
    if truth.rank == 0:
        assert np.all(got == 10.0) and np.all(g == mean) and f.log_c == 0.0


@pytest.mark.parametrize("name, truth", CASES, ids=[n for n, _ in CASES])
def test_lapack_route_reproduces_the_constructed_eigen_system(name, truth):
    """The yardstick of the GPU frame test, and the check that it is a fair one: the LAPACK route's rank is the constructed
    one and its frame-free deviations stay below the floor 64 * 2^-53 * lam_max / lam_min,kept, so 16 x yardstick or the
    floor is never a wide bound."""
    f = po.frame_from_cov(truth.cov)
    dev = po.frame_deviation(truth, f.U, f.A, f.log_c)
    print(f"{name:28s} rank {f.rank}  kappa {truth.kappa:9.3g}  dA {dev[0]:.2e}  dU {dev[1]:.2e}  dC {dev[2]:.2e}  floor {po.frame_floor(truth):.2e}")
    assert f.rank == truth.rank == po.frame_rank(f.U)
    assert max(dev) <= po.frame_floor(truth)


def test_sequential_moments_against_the_longdouble_oracle():
    rng = np.random.Generator(np.random.PCG64(8))
    for K in (1, 7, 30, 32):
        g = np.array([0.4, -1.2, 0.3]) + rng.standard_normal((K, 3)) * [0.05, 0.03, 0.01]
        w = rng.uniform(50, 400, size=K)
        mean, sigma, total = po.sequential_moments(g, w)
        m2, s2, t2 = orc.proposal_moments(g, w.astype(np.longdouble))
        np.testing.assert_allclose(mean, np.asarray(m2, dtype=np.float64), rtol=1e-13)
        np.testing.assert_allclose(sigma, np.asarray(s2, dtype=np.float64), rtol=1e-9, atol=1e-18)
        np.testing.assert_allclose(total, float(t2), rtol=1e-13)
        if K == 1:
            assert np.all(sigma == 0) and np.array_equal(mean, (g[0] * 1e-2) / 1e-2)
