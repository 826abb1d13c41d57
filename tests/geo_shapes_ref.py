"""Float64 restatements of the geometric structure embedding (csrc/geo.hip: PEM/model/transformer.py:259-363) and of the geometric score
term of the RPE self attention (csrc/rpe.hip: transformer.py:366-420), the seeded builders of tests/test_geo_shapes_gpu.py /
tests/test_geo_shapes_host.py and the table of bounds.  Plain numpy / torch on the CPU; of the product code only the two host-side
float64 helpers pem.cheb_coefficients and pem.geo_cheb_a_packed are used (the callers pass their results in), and both are checked in
the host test.

Two reference modes of the embedding row exist because every sinusoid kernel -- and the reference model itself -- forms the argument
idx * omega in fp32: at d_idx ~ 870 (the bg token) that rounding alone moves a row by 1.9e-5 against exact float64 products.  Pairs the
Chebyshev routes serve are compared with exact products (`arg32=False`), pairs a sinusoid kernel serves with the fp32 product
(`arg32=True`), each then evaluated in float64."""
import functools
import math
import types

import numpy as np
import torch

from oracle import pem_oracle as O

SIGMA_D = 0.2
XMAX = 24.0             # pem.GEO_XMAX: the Chebyshev range of the distance index
FLAG_LIMIT = 1.0e5      # common.h SAM6D_FAST_SINCOS_LIMIT: an index at or above it raises the range flag
H, C, K = 4, 256, 32

# Every bound is one the suite already holds the quantity to, or is derived in the function named.  Measured maxima over all cases of
# tests/test_geo_shapes_gpu.py (kernel on an MI355X / the fp32 oracle on the CPU, both against the float64 restatements of this file):
#   a_idx            kernel 9.5e-7 (1 ulp at 12; every kind and n)          bit recipe on the CPU vs the oracle 9.5e-7
#   rows, listed     fp16x3 1.8e-6, exact 2.9e-6 (both mm), flagged 2.4e-6  oracle 1.6e-6 (all), 1.5e-6 (mm), 2.6e-6 (indices to 3e5)
#   rows, routes     exact 3.1e-6, fp16x3 2.0e-6, Chebyshev 9.6e-7 on its own pairs (none), 1.9e-6 with listed ones   oracle 1.7e-6
#   cheb_vs_exact    3.9e-6 at scale 4.0 (all; bound 1.2e-5), 3.1e-6 at scale 4.8 (bg; bound 1.5e-5)
#   G                kernel 0.006 of g_bound (bg), query magnitudes 2^-60 .. 2^40 0.003                                oracle 0.008
#   P                kernel 0.005 of p_bound (5.4e-8 abs), row sums 0.13 of their bound, qk side effect 0.008 of g_bound  oracle 0.005
# g_bound is led by its first term, ||qp||_1 * TOL.rows: the kernels' rows are ten times inside TOL.rows.  Moving G64 itself (CPU,
# bg cloud, n = 65): dropping the c_lo . t_hi product of stage 1 moves 5 % of the in-range entries beyond g_bound (worst 1.7 of
# it), zeroing the one key of the last tile moves every entry of it beyond (at least 15.7 of it), swapping keys 63 and 64 likewise (7.6).
TOL = dict(
    a_idx=5e-6,           # angular indices vs the oracle: tests/test_pem_gpu.py::test_geo_indices_and_knn (max abs)
    rows=2e-5,            # embedding rows vs float64: test_geo_embedding_golden, non-bg pairs (max abs); with the fp32-argument
                          # reference the same bound holds for the listed and the flagged pairs
    cheb_vs_exact=3e-6,   # Chebyshev route vs exact kernel, x max(1, scale): test_geo_embedding_chebyshev_vs_sinusoid_kernels
)


def g_bound(qp, E64):
    """(Q,4,n) bound of |G - G64|: ||qp[q,h]||_1 * TOL.rows (the embedding error through the dot product) + 2^-20 * (sum_c |qp_c E_c| +
    qmax[q] * sum_c |E_c|): the fp32 accumulation, and the residual of the kernel's per-query power-of-two scaling and fp16 hi / lo
    split -- 2^-22 of qmax[q] = max |qp[q,:,:]|, taken four times."""
    q, e = qp.double().abs(), E64.double().abs()
    qmax = q.amax((1, 2))
    return (q.sum(2)[:, :, None] * TOL["rows"]
            + 2.0 ** -20 * (torch.einsum("qhc,qmc->qhm", q, e) + qmax[:, None, None] * e.sum(2)[:, None, :]))


def p_bound(P64, gb, score):
    """(Q,4,n) bound of |P - P64|: with delta = max_m g_bound / 8 + 2^-22 max |score| per row (the score's own error and its fp32
    rounding, the scaled difference and the exp2 argument), a probability moves by at most the factor e^(2 delta); the fp32 sum of n
    terms and the hardware exp add (n + 4) 2^-24 (pose_shapes_ref.sum_tol)."""
    n = P64.shape[-1]
    delta = gb.amax(2, keepdim=True) / 8.0 + 2.0 ** -22 * score.abs().amax(2, keepdim=True)
    return P64 * torch.expm1(2.0 * delta) + (n + 4) * 2.0 ** -24


def rowsum_tol(n):
    return (n + 4) * 2.0 ** -23


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------- weights
def weights(sd, p="geo_embedding"):
    """the embedding's parameters of a reference-keyed state_dict: fp32 as the model holds them, float64 copies for the restatements"""
    f = lambda k: sd[p + k].detach().float().cpu().contiguous()
    w = types.SimpleNamespace(div=f(".embedding.div_term"), Wd=f(".proj_d.weight"), bd=f(".proj_d.bias"), Wa=f(".proj_a.weight"),
                              ba=f(".proj_a.bias"))
    w.Wd64, w.Wa64, w.bias64 = w.Wd.double(), w.Wa.double(), w.bd.double() + w.ba.double()
    return w


def xmax_a(sigma_a):
    """pem.geo_cheb_a_packed's range of the angular indices: the angle is at most pi, plus 2^-6 of head room"""
    return min(XMAX, (180.0 / float(sigma_a)) * (1.0 + 2.0 ** -6))


def factor_a(sigma_a):
    return 180.0 / (sigma_a * math.pi)


# ------------------------------------------------------------------------------------------------------- indices
def dist32(points):
    """the fp32 distance matrix as geo_knn_kernel forms it: the correctly rounded sqrt of the bit-exact squared distance"""
    pd = O.pairwise_distance(points, points)
    return torch.sqrt(pd.double()).float()  # sqrt in float64, rounded once more: the correctly rounded fp32 root


def knn_stable(points):
    """(B,n,3) int64: entries 1..3 of a stable sort of every row of dist32 by (value, index) -- the kernel's documented tie rule"""
    return torch.sort(dist32(points), dim=2, stable=True).indices[:, :, 1:4]


def knn_tie_free(points):
    """(B,n) bool: the four smallest values of the row are distinct from each other and from the fifth"""
    v = torch.sort(dist32(points), dim=2).values[:, :, :5]
    return (v[:, :, 1:] != v[:, :, :-1]).all(2)


def d_idx_rounded(points, sigma_d=SIGMA_D):
    """d_idx = sqrt(pd) / sigma_d with both operations correctly rounded in fp32 (test_geo_indices_and_knn's assertion)"""
    root = dist32(points).double().numpy()
    return (root / np.float64(np.float32(sigma_d))).astype(np.float32)


def _fma(a, b, c):
    """fp32 fma through float64: the product of two fp32 values is exact there, the sum rounds to 53 bits and then to 24"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def a_idx_recipe(points, knn, sigma_a=15):
    """numpy restatement of geo_index_kernel's bit recipe of the angular indices -> (B,n,n,3) fp32"""
    p = points.numpy().astype(np.float32)
    B, n, _ = p.shape
    x = p[:, :, None, :]                                             # centre i
    anc = p[:, None, :, :] - x                                       # (B,n,n,3): p_j - p_i
    nb = np.take_along_axis(p[:, None, :, :].repeat(n, 1), knn.numpy()[:, :, :, None].repeat(3, 3), 2)  # (B,n,3,3): neighbours of i
    ref = nb - x                                                     # (B,n,3,3)
    out = np.empty((B, n, n, 3), np.float32)
    f32 = np.float32
    for r in range(3):
        r0, r1, r2 = (ref[:, :, r, c][:, :, None] + np.zeros((B, n, n), f32) for c in range(3))
        a0, a1, a2 = anc[..., 0], anc[..., 1], anc[..., 2]
        c0, c1, c2 = _fma(r1, a2, -(r2 * a1)), _fma(r2, a0, -(r0 * a2)), _fma(r0, a1, -(r1 * a0))
        s = np.sqrt(_fma(c2, c2, _fma(c1, c1, c0 * c0)).astype(np.float64)).astype(f32)
        c = (r0 * a0 + r1 * a1) + r2 * a2
        s = np.maximum(s, f32(1e-8))
        c = np.minimum(np.maximum(c, f32(-1.0) + f32(1e-8)), f32(1.0) - f32(1e-8))
        out[..., r] = np.arctan2(s.astype(np.float64), c.astype(np.float64)).astype(f32) * f32(factor_a(sigma_a))
    return out


def a_idx_oracle(points, knn, sigma_a=15):
    """the oracle's a_idx (O.geo_embedding_indices, PEM/model/transformer.py:322-341, the same fp32 torch operations) with the
    neighbours given: torch.topk orders tied distances arbitrarily, and a row whose neighbours tie (the dup kind) then holds its three
    angles in another order, or those of another neighbour.  Bit-equal to the oracle wherever the neighbours agree (host test)."""
    B, N, _ = points.shape
    k = knn.shape[2]
    knn_pts = torch.gather(points.unsqueeze(1).expand(B, N, N, 3), 2, knn.unsqueeze(3).expand(B, N, k, 3))
    ref = (knn_pts - points.unsqueeze(2)).unsqueeze(2).expand(B, N, N, k, 3)
    anc = (points.unsqueeze(1) - points.unsqueeze(2)).unsqueeze(3).expand(B, N, N, k, 3)
    sin_v = torch.clamp(torch.linalg.norm(torch.cross(ref, anc, dim=-1), dim=-1), min=1e-8)
    cos_v = torch.clamp(torch.sum(ref * anc, dim=-1), min=-1.0 + 1e-8, max=1.0 - 1e-8)
    return torch.atan2(sin_v, cos_v) * (180.0 / (sigma_a * math.pi))


def oracle_idx4(points, sigma_a=15):
    """(B,n,n,4) fp32 {d_idx, a_idx[0..2]} of the fp32 oracle"""
    d, a, _ = O.geo_embedding_indices(points, SIGMA_D, sigma_a, 3)
    return torch.cat([d[..., None], a], -1).contiguous()


# ------------------------------------------------------------------------------------------------------- embedding rows
def sinusoid64(x32, div, arg32):
    """(..., 256) float64 interleaved [sin, cos] of x * omega; arg32: the product rounded to fp32 first, as every sinusoid kernel (and
    the reference model) forms it"""
    arg = (x32.float()[..., None] * div.float()).double() if arg32 else x32.double()[..., None] * div.double()
    return torch.stack([torch.sin(arg), torch.cos(arg)], -1).reshape(*x32.shape, 2 * div.numel())


def rows64(idx4, w, arg32, chunk=8192):
    """the bias-free embedding row proj_d(sin/cos(d omega)) + max_k proj_a(sin/cos(a_k omega)) in float64 from fp32 indices (...,4)"""
    idx4 = torch.as_tensor(idx4, dtype=torch.float32)
    x = idx4.reshape(-1, 4)
    out = torch.empty(x.shape[0], C, dtype=torch.float64)
    for s in range(0, x.shape[0], chunk):
        e = sinusoid64(x[s:s + chunk], w.div, arg32)  # (c,4,256)
        out[s:s + chunk] = e[:, 0] @ w.Wd64.t() + (e[:, 1:] @ w.Wa64.t()).amax(1)
    return out.reshape(*idx4.shape[:-1], C)


def rows32(idx4, w):
    """the same row as the fp32 oracle computes it (O.sinusoidal_embedding and the two projections in float32, no bias)"""
    idx4 = torch.as_tensor(idx4, dtype=torch.float32)
    x = idx4.reshape(-1, 4)
    e = O.sinusoidal_embedding(x, w.div)  # (N,4,256) fp32
    return (e[:, 0] @ w.Wd.t() + (e[:, 1:] @ w.Wa.t()).amax(1)).reshape(*idx4.shape[:-1], C)


def classify(idx4, xmax, xa):
    """the boolean "listed" mask: any index outside [0, xmax] (d) or [0, xa] (a); NaN counts as outside"""
    v = torch.as_tensor(idx4, dtype=torch.float32)
    hi = torch.tensor([xmax, xa, xa, xa], dtype=torch.float32)
    return ~((v >= 0) & (v <= hi)).all(-1)


def rows64_served(idx4, w, listed):
    """rows64 as the Chebyshev routes serve them: exact products for the in-range pairs, the fp32 argument for the listed ones"""
    r = rows64(idx4, w, False)
    r[listed] = rows64(torch.as_tensor(idx4)[listed], w, True)
    return r


def scores64(qp, E64):
    """G64[q,h,m] = qp[q,h,:] . E64[q,m,:]   (E64 = rows64_served of idx4[q,m]; no per-row constant: the kernel's in-range term and the
    stored bias-free rows are the same quantity)"""
    return torch.einsum("qhc,qmc->qhm", qp.double(), E64)


def probs64(qk, G64):
    """softmax over m < n of (qk + G64) / 8 -> (probabilities, scores)"""
    s = (qk.double() + G64) / 8.0
    return torch.softmax(s, dim=2), s


# ------------------------------------------------------------------------------------------------------- clouds
KINDS = ("bg", "none", "all", "dup", "mm", "flag")


@functools.lru_cache(maxsize=None)
def cloud(kind, B, n, seed=0):
    """(B,n,3) fp32, seeded.
    bg:   unit cube, point 0 at (100,100,100): its row and column without their diagonal pair (d_idx = 0 exactly: 3 x 100^2 is exact
          in fp32), 2n - 2 pairs of every cloud, leave the Chebyshev range
    none: unit cube, no bg point: no pair does
    all:  n distinct points of a 7 x 7 x 7 lattice of spacing 6, jitter +-0.15: every off-diagonal pair does (d_idx >= 27)
    dup:  unit cube with points 0 and 1 bitwise equal, and the last three points on one line far from the cube, one and two steps of
          (1, 0.5, 1) from (5, 5, 5) (exact in fp32): they are each other's nearest neighbours, their cross products are exactly 0 (the
          1e-8 clamp) and their dot products 4.5 and -2.25 (both sides of the +-1 clamp); n = 4: point 0 = point 1 = the line's start
    mm:   cube of side 300 around (10, -20, 900): un-normalised millimetres, nearly every pair listed, flag clear
    flag: coordinates up to +-2e4: indices beyond the fast sincos range"""
    g = gen(1000 + 97 * KINDS.index(kind) + 7 * n + B + seed)
    pts = torch.rand(B, n, 3, generator=g)
    if kind == "bg":
        pts[:, 0] = 100.0
    elif kind == "all":
        for b in range(B):
            cell = torch.randperm(343, generator=g)[:n]
            lat = torch.stack([cell // 49, (cell // 7) % 7, cell % 7], 1).float() * 6.0
            pts[b] = lat + (pts[b] - 0.5) * 0.3
    elif kind == "dup":
        start, step = torch.tensor([5.0, 5.0, 5.0]), torch.tensor([1.0, 0.5, 1.0])
        for k in range(3):
            pts[:, n - 3 + k] = start + k * step
        pts[:, 0] = pts[:, 1]
    elif kind == "mm":
        pts = (pts - 0.5) * 300.0 + torch.tensor([10.0, -20.0, 900.0])
    elif kind == "flag":
        pts = (pts - 0.5) * 4.0e4
    return pts.contiguous()


# ------------------------------------------------------------------------------------------------------- crafted indices
EDGE_PERIOD = 11  # entries 0..7 of every run of 11 consecutive pairs are the special ones below, the rest random in-range indices


@functools.lru_cache(maxsize=None)
def edge(Q, n, xmax=XMAX, xa=None, seed=0):
    """(Q,n,4) fp32 indices fed to the ABI directly.  Pair (q,m) with (q n + m) % 11 = k holds
      0: all four exactly 0 (three equal angular indices: the max over k ties)       1: all four -0.0
      2: d = xmax exactly                                                            3: d = nextafter(xmax, +inf)        -> listed
      4: a_0 = xa exactly                                                            5: a_1 = nextafter(xa, +inf)        -> listed
      6: three equal random angular indices                                          7: d = xmax and all a = xa
    and the last key of every even query is listed (d = nextafter(xmax)), of every odd query in range: the last key of a partial key
    tile of 16 and, for n % 16 = 1, the only key of its tile."""
    xa = xmax_a(15) if xa is None else xa
    g = gen(5000 + 13 * Q + n + seed)
    f32 = np.float32
    v = torch.rand(Q * n, 4, generator=g).numpy().astype(f32)
    v[:, 0] *= f32(xmax * 0.999)
    v[:, 1:] *= f32(min(xa, 12.0))
    up_d, up_a = np.nextafter(f32(xmax), f32(np.inf)), np.nextafter(f32(xa), f32(np.inf))
    k = np.arange(Q * n) % EDGE_PERIOD
    v[k == 0] = 0.0
    v[k == 1] = -0.0
    v[k == 2, 0] = xmax
    v[k == 3, 0] = up_d
    v[k == 4, 1] = xa
    v[k == 5, 2] = up_a
    v[k == 6, 1:] = v[k == 6, 1:2]
    v[k == 7] = np.array([xmax, xa, xa, xa], f32)
    v = v.reshape(Q, n, 4)
    last = torch.rand(Q, 4, generator=g).numpy().astype(f32) * f32(min(xa, 12.0))
    last[0::2, 0] = up_d
    v[:, n - 1] = last
    return torch.from_numpy(v).contiguous()


def all_listed(pairs, seed=0):
    """(pairs,4) fp32: every distance index beyond the range (24.5 .. 900), angular indices in range"""
    g = gen(7000 + pairs + seed)
    v = torch.rand(pairs, 4, generator=g)
    v[:, 0] = 24.5 + v[:, 0] * 875.0
    v[:, 1:] *= 12.0
    return v.contiguous()


# ------------------------------------------------------------------------------------------------------- queries
def queries(Q, seed=0, l1=None):
    """qp (Q,4,256) fp32: randn; l1: every (query, head) row scaled to an L1 norm in [l1 / 2, l1]"""
    g = gen(9000 + Q + seed)
    qp = torch.randn(Q, H, C, generator=g)
    if l1 is not None:
        qp = qp / qp.abs().sum(2, keepdim=True) * (l1 * (0.5 + 0.5 * torch.rand(Q, H, 1, generator=g)))
    return qp.contiguous()


MAGNITUDES = ("2^-60", "1e-4", "1", "3e3", "2^40", "zero_query", "one_channel")


def magnitude_variant(qp, name):
    """the query-magnitude variants of the score test: a common factor, one all-zero query (query 1), one query (query 2) with a
    single channel 5e4 times the rest"""
    qp = qp.clone()
    if name == "zero_query":
        qp[1] = 0.0
    elif name == "one_channel":
        qp[2, :, 37] *= 5.0e4
    else:
        qp *= {"2^-60": 2.0 ** -60, "1e-4": 1e-4, "1": 1.0, "3e3": 3e3, "2^40": 2.0 ** 40}[name]
    return qp.contiguous()


def fold_qd(qp, dc):
    """qd = fp32(qp64 @ D_c): the query folded into proj_d's Chebyshev coefficients dc (256,32) float64, formed in float64"""
    return (qp.double().reshape(-1, C) @ torch.as_tensor(dc, dtype=torch.float64)).float().reshape(-1, K).contiguous()


def cheb_eval(c, x, xmax):
    """sum_p c[:, p] T_p(2 x / xmax - 1) in float64: c (cols,K), x (N,) -> (N,cols)"""
    u = 2.0 * np.asarray(x, np.float64) / xmax - 1.0
    return np.polynomial.chebyshev.chebval(u, np.asarray(c, np.float64).T).T
