"""The inputs and bounds of tests/test_geo_shapes_gpu.py, proved on the CPU: the seeded builders of tests/geo_shapes_ref.py list the
pairs they promise, the float64 restatements agree with the golden cloud and with the fp32 oracle (oracle/pem_oracle.py), and the
oracle alone meets every bound of the TOL table -- so the GPU file encodes no bound the reference arithmetic itself would miss.  The
two host-side float64 helpers of the product the GPU file relies on (pem.cheb_coefficients, pem.geo_cheb_a_packed) are checked here."""
import numpy as np
import pytest
import torch

from tests import geo_shapes_ref as R
from tests._util import golden
from oracle import pem_oracle as O


@pytest.fixture(scope="module")
def sd():
    from sam6d_hip import synth
    return synth.make_pem_weights(1)


@pytest.fixture(scope="module")
def w(sd):
    return R.weights(sd)


def _err(got, want):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    return float((got - want).abs().max()) if got.numel() else 0.0


# ------------------------------------------------------------------------------------------------------- kNN
def test_knn_stable_reproduces_the_golden_cloud():
    g = golden("geo_embedding")
    pts = torch.from_numpy(g["pts"])
    assert np.array_equal(R.knn_stable(pts).numpy(), g["knn"].astype(np.int64))


@pytest.mark.parametrize("kind,B,n", [("bg", 3, 4), ("bg", 1, 64), ("bg", 3, 65), ("bg", 1, 256), ("none", 3, 5), ("none", 1, 197),
                                      ("all", 3, 129), ("dup", 3, 63), ("mm", 1, 255)])
def test_knn_stable_equals_topk_without_ties(kind, B, n):
    pts = R.cloud(kind, B, n)
    free = R.knn_tie_free(pts)
    got, want = R.knn_stable(pts), O.geo_embedding_indices(pts)[2]
    print("%s B %d n %d: %d of %d rows tie-free" % (kind, B, n, int(free.sum()), free.numel()))
    assert torch.equal(got[free], want[free])
    if kind in ("bg", "none", "all"):
        assert bool(free.all()), "the random builders have no tie among the four smallest distances of a row"
    if kind == "dup":
        assert not bool(free[:, 0].any()) and not bool(free[:, 1].any()), "the bitwise duplicates tie with their own diagonal entry"
        assert torch.equal(got[:, 0, 0], torch.ones(B, dtype=torch.int64)), "point 0: {0, 1} tie at the front, so entry 1 is point 1"
        assert torch.equal(got[:, 1, 0], torch.ones(B, dtype=torch.int64)), "point 1: the stable order is 0, 1: entry 1 is itself"


# ------------------------------------------------------------------------------------------------------- angular indices
@pytest.mark.parametrize("kind,n", [("bg", 4), ("bg", 5), ("bg", 17), ("bg", 64), ("bg", 197), ("bg", 256), ("none", 65), ("all", 65),
                                    ("mm", 65)])
def test_index_recipe_vs_oracle(kind, n):
    """the kernel's bit recipe restated in numpy stays within 1 ulp (9.6e-7 at 12) of the oracle's a_idx, so TOL.a_idx (5e-6) holds
    off the golden shape for the reference alone (0.5 ulp for the lattice, 0 for the millimetre cube, whose dot products all clamp);
    d_idx of the oracle is within 2 ulp of the correctly rounded one"""
    pts = R.cloud(kind, 2 if n <= 65 else 1, n)
    d, a, knn = O.geo_embedding_indices(pts)
    assert torch.equal(knn, R.knn_stable(pts)) and torch.equal(R.a_idx_oracle(pts, knn), a), "a_idx_oracle is the oracle, neighbours given"
    got = R.a_idx_recipe(pts, R.knn_stable(pts))
    e = float(np.abs(got.astype(np.float64) - a.numpy().astype(np.float64)).max())
    print("%s n %d: a_idx recipe vs oracle %.2e (1 ulp 9.6e-7, bound %.1e)" % (kind, n, e, R.TOL["a_idx"]))
    assert e <= 9.6e-7
    ulp = np.abs(R.d_idx_rounded(pts).view(np.int32).astype(np.int64) - d.numpy().view(np.int32).astype(np.int64))
    assert ulp.max() <= 2


@pytest.mark.parametrize("n", [4, 63, 256])
def test_index_recipe_vs_oracle_with_tied_neighbours(n):
    """dup: the middle point of the line has its two neighbours at the same distance, and the duplicates tie with themselves; the
    oracle's topk orders them arbitrarily (angles of pi and 0 trade places: 12 apart), so a_idx is compared with the oracle's
    arithmetic on the neighbours of the documented tie rule -- and there the bit recipe stays within 1 ulp as well"""
    pts = R.cloud("dup", 3, n)
    knn = R.knn_stable(pts)
    a = R.a_idx_oracle(pts, knn)
    e = float(np.abs(R.a_idx_recipe(pts, knn).astype(np.float64) - a.numpy().astype(np.float64)).max())
    print("dup n %d: a_idx recipe vs oracle arithmetic on the stable neighbours %.2e" % (n, e))
    assert e <= 9.6e-7
    mid = a[:, n - 2, n - 1]  # centre = the line's middle point, anchor = its end: one neighbour is the end (0), one the start (pi)
    assert float(mid.min()) < 1e-6 and abs(float(mid.max()) - 12.0) < 2e-6, "both sides of the +-1 clamp, the 1e-8 clamp under them"


# ------------------------------------------------------------------------------------------------------- listed pairs
@pytest.mark.parametrize("B,n", [(3, 4), (2, 65), (1, 256)])
def test_listed_counts_of_the_builders(B, n):
    xa = R.xmax_a(15)
    assert abs(xa - 12.1875) < 1e-12
    count = lambda kind: int(R.classify(R.oracle_idx4(R.cloud(kind, B, n)), R.XMAX, xa).sum())
    # the bg point's row and column; its own diagonal pair has d_idx = 0 (30000 - 2 * 30000 + 30000 is exact) and a_idx = 6 (anc = 0)
    assert count("bg") == B * (2 * n - 2)
    assert count("none") == 0
    amax = float(R.oracle_idx4(R.cloud("none", B, n))[..., 1:].max())
    print("none B %d n %d: largest a_idx %.6f" % (B, n, amax))
    assert amax < xa
    idx = R.oracle_idx4(R.cloud("all", B, n))
    listed = R.classify(idx, R.XMAX, xa)
    eye = torch.eye(n, dtype=torch.bool).expand(B, n, n)
    assert int(listed.sum()) == B * (n * n - n) and not bool(listed[eye].any())
    assert float(R.oracle_idx4(R.cloud("flag", B, n)).max()) >= R.FLAG_LIMIT
    mm = R.oracle_idx4(R.cloud("mm", B, n))
    assert float(mm.max()) < R.FLAG_LIMIT
    share = float(R.classify(mm, R.XMAX, xa).float().mean())
    assert share >= 1.0 - 1.5 / n, "mm: nearly every off-diagonal pair is listed (share %.4f)" % share


def test_classify_and_edge_builder():
    xa = R.xmax_a(15)
    nan = torch.tensor([[1.0, float("nan"), 1.0, 1.0], [float("nan"), 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0], [-0.0, -0.0, 0.0, 0.0],
                        [-1e-30, 1.0, 1.0, 1.0], [24.0, xa, xa, xa], [1.0, 12.5, 1.0, 1.0], [12.5, 1.0, 1.0, 1.0]])
    assert R.classify(nan, R.XMAX, xa).tolist() == [True, True, False, False, True, False, True, False]
    for Q, n in [(1, 4), (17, 17), (5, 209), (2, 256)]:
        v = R.edge(Q, n)
        listed = R.classify(v, R.XMAX, xa)
        k = (torch.arange(Q * n) % R.EDGE_PERIOD).reshape(Q, n)
        want = (k == 3) | (k == 5)
        want[:, n - 1] = torch.arange(Q) % 2 == 0
        assert torch.equal(listed, want)
        flat = v.reshape(-1, 4)
        kk = k.reshape(-1)
        body = torch.ones(Q, n, dtype=torch.bool)
        body[:, n - 1] = False
        body = body.reshape(-1)
        if int(((kk == 1) & body).sum()):
            assert bool(torch.signbit(flat[(kk == 1) & body]).all()), "-0.0 entries keep their sign"
        if int(((kk == 2) & body).sum()):
            assert bool((flat[(kk == 2) & body, 0] == 24.0).all())
        if int(((kk == 6) & body).sum()):
            t = flat[(kk == 6) & body]
            assert bool((t[:, 1] == t[:, 2]).all() and (t[:, 2] == t[:, 3]).all())
        assert float(v[0, n - 1, 0]) == float(np.nextafter(np.float32(24.0), np.float32(np.inf)))
    v = R.all_listed(257)
    assert bool(R.classify(v, R.XMAX, R.XMAX).all())


# ------------------------------------------------------------------------------------------------------- embedding rows
def _index_classes():
    g = R.gen(3)
    bg = R.oracle_idx4(R.cloud("bg", 2, 65))
    far = bg[:, 0, 1:]  # the bg point's pairs: d_idx ~ 870
    assert float(far[..., 0].min()) > 800.0
    return {
        "in-range": (R.oracle_idx4(R.cloud("none", 2, 65)).reshape(-1, 4), 2.6e-6),
        "d ~ 870": (far.reshape(-1, 4), 3.2e-6),
        "up to 3e5": (R.oracle_idx4(R.cloud("flag", 2, 40)).reshape(-1, 4), 3.1e-6),
        "edge set": (R.edge(17, 65, R.XMAX, R.XMAX).reshape(-1, 4), 1.2e-6),
        "random to 24": (torch.rand(4096, 4, generator=g) * 24.0, None),
    }


def test_fp32_oracle_rows_meet_the_bound(w):
    """the fp32 oracle alone against rows64 with the fp32 argument: within TOL.rows for every index class, the far and flagged ones
    included; against exact float64 products the d ~ 870 rows are off by about the bound itself -- hence the two reference modes"""
    for name, (idx, measured) in _index_classes().items():
        e = _err(R.rows32(idx, w), R.rows64(idx, w, True))
        print("%-12s fp32 oracle vs rows64(arg32=True): %.2e (bound %.1e, measured when written: %s)" % (name, e, R.TOL["rows"], measured))
        assert e <= R.TOL["rows"] / 4, "the oracle keeps a factor of four below the bound on every class"
    far = _index_classes()["d ~ 870"][0]
    plain = _err(R.rows32(far, w), R.rows64(far, w, False))
    print("d ~ 870      fp32 oracle vs rows64(arg32=False): %.2e" % plain)
    assert plain > 1e-5, "at d ~ 870 the fp32 rounding of idx * omega alone is worth half the bound"
    near = _index_classes()["in-range"][0]
    both = _err(R.rows64(near, w, False), R.rows64(near, w, True))
    print("in-range     rows64(arg32=False) vs rows64(arg32=True): %.2e" % both)
    assert both <= R.TOL["rows"] / 4, "in range the two modes agree far inside the bound"


def test_rows64_bias_and_max(w):
    """rows64 against a direct float64 transcription of the model on a handful of pairs: interleaved [sin, cos], max over the 3 angular rows"""
    idx = R.edge(1, 17, R.XMAX, R.XMAX)[0]
    got = R.rows64(idx, w, False)
    for m in range(17):
        x = idx[m].double()
        emb = torch.zeros(4, 256, dtype=torch.float64)
        emb[:, 0::2] = torch.sin(x[:, None] * w.div.double())
        emb[:, 1::2] = torch.cos(x[:, None] * w.div.double())
        want = w.Wd64 @ emb[0] + torch.stack([w.Wa64 @ emb[k] for k in (1, 2, 3)]).amax(0)
        assert _err(got[m], want) < 1e-13


# ------------------------------------------------------------------------------------------------------- score term
@pytest.mark.parametrize("kind", ["bg", "none", "all", "edge", "dup", "mm", "flag"])
def test_fp32_einsum_meets_g_bound(w, kind):
    """G as the fp32 oracle would form it (fp32 rows, a float32 einsum with the folded query) is inside g_bound for every builder and
    every query-magnitude variant"""
    n, B = 65, 1
    xa = R.xmax_a(15)
    idx = R.edge(B * n, n) if kind == "edge" else R.oracle_idx4(R.cloud(kind, B, n)).reshape(B * n, n, 4)
    listed = R.classify(idx, R.XMAX, xa)
    E64 = R.rows64_served(idx, w, listed)
    E32 = R.rows32(idx, w)
    base = R.queries(B * n)
    for name in R.MAGNITUDES:
        qp = R.magnitude_variant(base, name)
        G64, gb = R.scores64(qp, E64), R.g_bound(qp, E64)
        G32 = torch.einsum("qhc,qmc->qhm", qp, E32)
        ratio = float(((G32.double() - G64).abs() / gb.clamp_min(1e-300)).max())
        print("%s %-12s fp32 einsum: max |G32 - G64| / g_bound = %.3f" % (kind, name, ratio))
        assert ratio <= 1.0
        if name == "zero_query":
            assert float(gb[1].max()) == 0.0 and float(G64[1].abs().max()) == 0.0


def test_p_bound_holds_for_the_fp32_softmax(w):
    n, B = 65, 1
    idx = R.oracle_idx4(R.cloud("bg", B, n)).reshape(B * n, n, 4)
    listed = R.classify(idx, R.XMAX, R.xmax_a(15))
    E64 = R.rows64_served(idx, w, listed)
    qp = R.queries(B * n, l1=8.0)
    assert float(qp.abs().sum(2).max()) <= 8.0 * (1 + 1e-6)
    qk = torch.randn(B * n, R.H, n, generator=R.gen(5)) * 4.0
    G64 = R.scores64(qp, E64)
    P64, s = R.probs64(qk, G64)
    pb = R.p_bound(P64, R.g_bound(qp, E64), s)
    P32 = torch.softmax((qk + torch.einsum("qhc,qmc->qhm", qp, R.rows32(idx, w))) * 0.125, dim=2)
    ratio = float(((P32.double() - P64).abs() / pb).max())
    print("fp32 softmax: max |P32 - P64| / p_bound = %.3f" % ratio)
    assert ratio <= 1.0
    assert float((P32.double().sum(2) - 1).abs().max()) <= R.rowsum_tol(n)


# ------------------------------------------------------------------------------------------------------- Chebyshev helpers
def test_chebyshev_expansions_on_the_closed_range(sd, w):
    """pem.cheb_coefficients reproduces the projected sinusoid to <= 1e-10 on the whole closed range, both end points included;
    pem.geo_cheb_a_packed picks 2 stage-1 products for sigma_a = 15 and 3 for 7.5, and its image holds the coefficients x 1024"""
    from sam6d_hip import pem
    W = pem.pack_geo(sd, torch.device("cpu"))
    xa = R.xmax_a(15)
    for name, Wm, xmax, measured in (("proj_d", w.Wd, R.XMAX, 3.8e-12), ("proj_a", w.Wa, xa, 1.6e-14)):
        c = pem.cheb_coefficients(Wm, w.div, xmax=xmax)
        assert c.shape == (256, 32) and c.dtype == np.float64
        x = np.concatenate([np.linspace(0.0, xmax, 4001), [0.0, xmax, float(np.nextafter(np.float32(xmax), np.float32(0)))]])
        want = (R.sinusoid64(torch.from_numpy(x), w.div.double(), False) @ Wm.double().t()).numpy()
        e = float(np.abs(R.cheb_eval(c, x, xmax) - want).max())
        print("%s on [0, %g]: Chebyshev vs projected sinusoid %.2e (measured when written: %.1e)" % (name, xmax, e, measured))
        assert e <= 1e-10
    img, xa15, products, fits = pem.geo_cheb_a_packed(W, 15)
    assert (xa15, products, fits) == (xa, 2, True)
    img75, xa75, products75, fits75 = pem.geo_cheb_a_packed(W, 7.5)
    assert (xa75, products75, fits75) == (24.0, 3, True)
    c = pem.cheb_coefficients(w.Wa, w.div, xmax=xa) * 1024.0
    hi, lo = img[:, :32].float().double().numpy(), img[:, 32:64].float().double().numpy()
    assert img.shape == (256, 72) and img.dtype == torch.float16 and float(img[:, 64:].abs().max()) == 0.0
    assert float(np.abs(hi + lo - c).max()) <= 2.0 ** -22 * float(np.abs(c).max()), "hi + lo carries the coefficient to fp16 x 2 precision"
