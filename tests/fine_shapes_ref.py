"""Float64 restatement of the fused fine-match pipeline (csrc/finematch.hip: PEM/utils/model_utils.py:131-153 compute_feature_similarity
and :308-331, the head of compute_fine_Rt), the seeded input builders of tests/test_fine_shapes_gpu.py / tests/test_fine_shapes_host.py
and the table of bounds.  Plain torch on the CPU; no GPU, no product code.  first_argmax, assign64, sum_tol, LABEL_REL and LABEL_SHARE
are the pose module's (tests/pose_shapes_ref.py).

The pipeline differs from the launch-per-op kernels in its arithmetic: no running maximum but the fixed shift c = 1 / temp, operands cut
into fp16 hi / lo halves of unit vectors x 2^10, per-tile partial sums merged in a fixed order, hardware exp2 / rcp.  An arg-max is
compared exactly only where the float64 values clear the decision by label_rel(temp); the labels left out (`near`) must still be one of
the float64 candidates within that margin, and a case may leave out at most LABEL_SHARE of its rows and of its columns -- a condition on
the INPUTS, which the host test asserts for every case.

Ties against the bg row or bg column are not built: fm_bg_kernel computes those entries as a wave-wide dot product of hi + lo, not on
the matrix cores, so a duplicate of the bg token is not a bitwise tie in the kernel."""
import functools

import torch

from tests.pose_shapes_ref import LABEL_REL, LABEL_SHARE, assign64, first_argmax, gen, sum_tol  # noqa: F401  (re-exported to the two test files)

C = 256
LOG2E = 1.4426950408889634
# the smallest temperature of the fixed shift: E = exp2((cos - 1) log2e / temp) reaches its smallest exponent -2 log2e / temp at cos = -1;
# exp2 flushes results below 2^-126, and one unit of margin covers the rounding of the fmaf and a |cos| of 1 + 1e-6
MIN_TEMP = 2.0 * LOG2E / 125.0
TEMPS = (1.0, 0.1, 0.03)
# A row or column whose float64 maximum of S lies below the smallest normal float32 is beyond float32 itself: the product of the two
# softmaxes is a subnormal there, in the kernel as in the reference's own float32 (the float32 restatement disagrees with float64 on such
# rows too), so its label is only required to be a valid index.  Only `antipodal` has such rows -- the 64 that point away from every
# template row: softmax(att, 1) of their entries is e^(-2 / MIN_TEMP) = 2^-125 -- and the host test asserts exactly that.
S_NORMAL = 2.0 ** -126
N = 2049


# ------------------------------------------------------------------------------------------------------------------ bounds
def att_tol(temp, mode=1):
    """absolute bound of the pipeline's att = cos / temp against float64, from float32 features.  In units of the cosine:

    mode 1 (three fp16 products hi.hi + hi.lo + lo.hi of operands x = unit vector * 2^10):
      * representation: hi = fp16(x), lo = fp16(x - hi): |x - hi - lo| <= 2^-11 |x - hi| <= 2^-22 |x| where lo is a normal fp16, and
        <= 2^-25 (half a subnormal step) elsewhere: an operand's error vector has norm <= 2^-22 * 2^10 + 2^-25 * sqrt(256) in the scaled
        units = 2^-22 + 2^-31 of the unit vector; by Cauchy-Schwarz the dot product of two such operands moves by <= 2 (2^-22 + 2^-31)
      * the dropped lo.lo product: |lo| <= 2^-11 |x| per operand -> <= 2^-22 by Cauchy-Schwarz
      * fp32 accumulation: every fp16 x fp16 product is exact in fp32; the 768 of them are summed in 48 v_mfma steps of 16 terms each.
        A blocked sum errs by <= (block + blocks) 2^-24 sum |terms|, and sum |a_k b_k| <= 1 (Cauchy-Schwarz): (16 + 48) 2^-24 = 2^-18
      * the float32 normalisation: 256 squares summed by a tree (9 roundings on a sum of positive terms, halved by the square root), the
        square root and the division round once each: a component is off by <= 6.5 * 2^-24 relative, the cosine by twice that
      * the exponent: k1 = log2e / (2^20 temp) and k2 = log2e / temp are rounded to float32 and fmaf rounds once; the exponent's size
        is <= 2 log2e / temp: 3 roundings * 2 * 2^-24 in units of the cosine
    mode 2 (hi.hi only): each operand is off by <= 2^-11 relative -> 2^-10 (the other terms, 5e-6, are the slack of the worst case:
      2^-11 is reached only by a component at the bottom of its binade, never by 256 of them at once)."""
    if mode == 2:
        return 2.0 ** -10 / temp
    rep = 2.0 * (2.0 ** -22 + 2.0 ** -31)
    lolo = 2.0 ** -22
    acc = (16 + 48) * 2.0 ** -24
    norm = 2.0 * 6.5 * 2.0 ** -24
    expo = 3 * 2.0 * 2.0 ** -24
    return (rep + lolo + acc + norm + expo) / temp


def chain_att_tol(temp):
    """att_tol of the sam6d_linear_norm_split -> sam6d_fine_match_split chain: the suite holds every component of fh + fl to 3e-7 of the
    float64 unit vector (tests/test_block_gpu.py::test_linear_norm_split_vs_fp64), so an operand is off by <= 3e-7 * sqrt(256) in norm
    and the cosine by twice that; the product's own terms (lo.lo, accumulation, exponent) as in att_tol"""
    return (2.0 * 3e-7 * 16.0 + 2.0 ** -22 + (16 + 48) * 2.0 ** -24 + 3 * 2.0 * 2.0 ** -24) / temp


def label_rel(temp, tol=None):
    """S = E^2 / (rsum csum): an error e of att moves E^2 by 2 e relative and each of the two sums by <= e -> 4 att_tol, plus the pose
    module's LABEL_REL for the hardware exp2 / rcp"""
    return 4.0 * (att_tol(temp) if tol is None else tol) + LABEL_REL


# 4 x the relative error of the float32 CPU restatement (oracle.pem_oracle.soft_assignment + the mask) against float64 on the same
# inputs: tests/test_fine_shapes_host.py measures it per case and asserts it stays below the entry here (weights, targets):
# measured (the larger of weights and targets), temp 1.0 / 0.1 / 0.03: matched 3.0e-7 / 5.6e-6 / 6.1e-9, flat 2.8e-7 / 3.8e-7 / 8.8e-6,
# all_bg 0 / 0 / 0, no_bg 3.3e-7 / 4.7e-6 / 9.6e-10, ranges 2.7e-7 / 4.8e-6 / 1.6e-6; n = 4097 at 0.1: matched 6.0e-6, flat 3.9e-7;
# at MIN_TEMP: antipodal 5.4e-6, flat 9.6e-6 -- an entry of the table is the largest of its temperature, rounded up
F32_REL = {1.0: 4e-7, 0.1: 7e-6, 0.03: 1e-5, MIN_TEMP: 1e-5}


def weight_rel(temp, n, tol=None):
    """relative bound of weight[n] = sum_m A[n][m]: the larger of
      * derived: the numerator E^2 of every term moves by 2 att_tol; the two softmax denominators are fp32 sums of n positive terms
        (sum_tol(n) each, any order: the tile partials and their merges are one such order)
      * 4 x the float32 restatement's own error (F32_REL; the factor covers the hardware exp2 / rcp at about 1e-6 a factor)"""
    derived = 2.0 * (att_tol(temp) if tol is None else tol) + 2.0 * sum_tol(n)
    f32 = 4.0 * F32_REL[min(F32_REL, key=lambda t: abs(t - temp))]
    return max(derived, f32)


def weight_floor(n):
    """what a relative bound cannot cover: a factor E * (1 / rsum) or the product of the two factors below 2^-126 is flushed to zero,
    one such loss per term of the row"""
    return n * 2.0 ** -125


def target_floor(n):
    """pred = sum_m A p / (weight + 1e-6): the flushed terms of weight_floor over the smallest denominator, and the float32 rounding of
    the quotient (|pred| <= 0.5).  The relative part is weight_rel * 0.5: weights moved by a factor 1 +- rel move their weighted mean
    by rel times the mean absolute deviation of p, and a variable confined to [-0.5, 0.5] has one of at most 0.5."""
    return weight_floor(n) / 1e-6 + 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ float64
def normalize64(x):
    """F.normalize (model_utils.py:141-142): x / max(|x|, 1e-12) in float64"""
    x = x.double()
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def chain64(x, W, b):
    """FinePointMatching's out_proj (PEM/model/fine_point_matching.py:70-72) x W^T + b in float64, then normalize64: the reference of
    the sam6d_linear_norm_split -> sam6d_fine_match_split chain.  The result is already normalised (fine_match64 normalises again,
    which changes a float64 unit vector by 1e-16)."""
    return normalize64(x.double() @ W.double().t() + b.double())


def att64(F, b, B, temp):
    """float64 att (n, n) of proposal b from the features F (2B, n, 256) (float32 features or chain64's float64 rows)"""
    return normalize64(F[b]) @ normalize64(F[B + b]).t() / temp


def _one64(att, rel):
    a = att
    er, ec = torch.exp(a - a.max(1, keepdim=True).values), torch.exp(a - a.max(0, keepdim=True).values)
    S = (er / er.sum(1, keepdim=True)) * (ec / ec.sum(0, keepdim=True))  # softmax(att, 2) * softmax(att, 1)
    out = {}
    for key, X in (("1", S[1:, :]), ("2", S[:, 1:].t())):  # rows of X: the entries the label is the arg-max of
        top = torch.topk(X, 3, dim=1).values
        near = (top[:, 0] - top[:, 1]) <= rel * top[:, 0]
        out["l" + key] = first_argmax(X, 1)
        out["near" + key] = near
        out["tiny" + key] = top[:, 0] < S_NORMAL
        out["cand" + key] = {int(i): torch.nonzero(X[i] >= top[i, 0] * (1.0 - rel))[:, 0] for i in torch.nonzero(near)[:, 0]}
        out["third" + key] = top
    return out


def fine_match64(F, B, temp, pts2=None, rel=None):
    """model_utils.py:131-153 and :308-331 in float64 from the features F (2B, n, 256), one proposal at a time -> dict of l1, l2
    (B, n-1) first arg-max labels, near1, near2 (B, n-1): the two best float64 values of the row / column lie within `rel` (default
    label_rel(temp)) of each other, cand1, cand2: per proposal {index: the float64 candidates within rel of the maximum} of the near
    rows / columns, top1, top2 (B, n-1, 3): the three best values.  With pts2 also weight, pred of the float64 labels (assign64)."""
    rel = label_rel(temp) if rel is None else rel
    per = []
    for b in range(B):
        o = _one64(att64(F, b, B, temp), rel)
        if pts2 is not None:
            w = assign64(att64(F, b, B, temp)[None], o["l1"][None], o["l2"][None], pts2[b][None])
            o["weight"], o["pred"] = w["weight"][0], w["pred"][0]
        per.append(o)
    out = {k: torch.stack([o[k] for o in per]) for k in ("l1", "l2", "near1", "near2", "tiny1", "tiny2") + (("weight", "pred") if pts2 is not None else ())}
    out["cand1"], out["cand2"] = [o["cand1"] for o in per], [o["cand2"] for o in per]
    out["top1"], out["top2"] = torch.stack([o["third1"] for o in per]), torch.stack([o["third2"] for o in per])
    return out


def assign_from(F, B, temp, l1, l2, pts2):
    """weight (B, n-1), pred (B, n-1, 3) in float64 from GIVEN labels (those of the implementation under test), one proposal at a time"""
    ws, ps = [], []
    for b in range(B):
        w = assign64(att64(F, b, B, temp)[None], l1[b][None].long(), l2[b][None].long(), pts2[b][None])
        ws.append(w["weight"][0])
        ps.append(w["pred"][0])
    return torch.stack(ws), torch.stack(ps)


# ------------------------------------------------------------------------------------------------------------------ builders
KINDS = ("matched", "flat", "all_bg", "no_bg", "ranges")
RANGE_SCALES = (1e-12, 1.0, 1e12)
ZERO_ROWS = (5, 7)          # (scene row, template row) of `ranges` set to exact zeros
ANTIPODAL_ROWS = (1, 65)    # scene rows of `antipodal` that point away from every template row


def _matched(g, n, bg_third=True, noise=0.25):
    tpl = torch.randn(n, C, generator=g)
    perm = torch.randperm(n, generator=g)
    src = tpl[perm].clone()
    if bg_third:
        src[::3] = tpl[0]  # every third scene row looks like the template's bg token
    return src + noise * torch.randn(n, C, generator=g), tpl


def proposal(kind, n, seed):
    """-> scene (n, 256), template (n, 256), pts2 (n-1, 3) of one proposal; every draw comes from one generator seeded by (kind, n, seed)"""
    g = gen(7000 + 131 * seed + n + 17 * (KINDS + ("antipodal", "plain")).index(kind))
    if kind in ("matched", "ranges"):
        scn, tpl = _matched(g, n)
    elif kind == "plain":  # matched pairs only: the base of the tie cases
        scn, tpl = _matched(g, n, bg_third=False)
    elif kind == "flat":
        scn, tpl = torch.randn(n, C, generator=g), torch.randn(n, C, generator=g)
    elif kind == "all_bg":
        tpl = torch.randn(n, C, generator=g)
        scn = tpl[0][None] + 0.25 * torch.randn(n, C, generator=g)
    elif kind == "no_bg":
        tpl = torch.randn(n, C, generator=g)
        perm = torch.randperm(n - 1, generator=g) + 1
        scn = torch.empty(n, C)
        scn[1:] = tpl[perm] + 0.25 * torch.randn(n - 1, C, generator=g)
        scn[0], tpl[0] = -scn[1:].mean(0), -tpl[1:].mean(0)
    elif kind == "antipodal":
        u = 0.25 * torch.randn(C, generator=g)  # |u| = 4: the 0.32-long noise leaves cos = -0.994 and still tells the template rows apart
        tpl = u[None] + 0.02 * torch.randn(n, C, generator=g)
        perm = torch.randperm(n, generator=g)
        scn = tpl[perm] + 0.005 * torch.randn(n, C, generator=g)
        lo, hi = ANTIPODAL_ROWS
        scn[lo:hi] = -u[None] + 0.02 * torch.randn(hi - lo, C, generator=g)
    else:
        raise KeyError(kind)
    if kind == "ranges":
        s = torch.tensor(RANGE_SCALES)[torch.arange(n) % 3][:, None]
        scn, tpl = scn * s, tpl * s
        scn[ZERO_ROWS[0]] = 0.0
        tpl[ZERO_ROWS[1]] = 0.0
    pts2 = torch.rand(n - 1, 3, generator=g) - 0.5
    return scn, tpl, pts2


def stack(props):
    """[(scene, template, pts2)] -> F (2B, n, 256) [scene clouds; template clouds], pts2 (B, n-1, 3)"""
    return (torch.stack([p[0] for p in props] + [p[1] for p in props]).contiguous(), torch.stack([p[2] for p in props]).contiguous())


def _merge(per):
    keys = [k for k in per[0] if not k.startswith("cand")]
    out = {k: torch.cat([o[k] for o in per]) for k in keys}
    out["cand1"], out["cand2"] = [o["cand1"][0] for o in per], [o["cand2"][0] for o in per]
    return out


@functools.lru_cache(maxsize=48)
def proposal64(kind, n, seed, temp):
    """fine_match64 (with weight / pred of its own labels) of one seeded proposal, computed once per process and left unchanged"""
    scn, tpl, pts2 = proposal(kind, n, seed)
    return fine_match64(torch.stack([scn, tpl]), 1, temp, pts2[None])


def case(kind, temp, n=N, seeds=(0, 1)):
    """(F, pts2, float64 result) of one builder: proposal b is proposal(kind, n, seeds[b]), whatever the rest of the batch"""
    F, pts2 = stack([proposal(kind, n, s) for s in seeds])
    return F, pts2, _merge([proposal64(kind, n, s, temp) for s in seeds])


# (axis, name, n, first, second, where): `second` is a bitwise copy of `first`; `where` is the scene row (axis "tpl": template rows
# duplicated, l1[where] must be `first`) or the template row (axis "scn": scene rows duplicated, l2[where] must be `first`) that is a
# noisy copy of the duplicated row.  A lane of the label pass owns columns 1 + 4 (lane + 64 g) + j, g < 8, j < 4; wave w of a
# 64-row slab takes rows 1 + 64 slab + w + 4 k.
TIE_CASES = [
    ("tpl", "same_group_of_four", N, 553, 554, 300),    # lane 10, g = 2, j = 0 and 1
    ("tpl", "same_lane_next_group", N, 553, 809, 301),  # lane 10, g = 2 and 3
    ("tpl", "neighbouring_lanes", N, 553, 557, 302),    # lanes 10 and 11
    ("tpl", "lane_63_then_lane_0", N, 254, 258, 303),   # the lower column in lane 63 (g = 0), the higher in lane 0 (g = 1)
    ("tpl", "gemm_tile_edge", N, 128, 129, 304),        # the last column of tile 0 and the first of tile 1
    ("tpl", "chunk_merge", 4097, 553, 2601, 300),       # the same lane slot of the two 2048-column chunks
    ("scn", "same_wave", N, 70, 74, 300),               # wave 1, k = 1 and 2 of slab 1
    ("scn", "another_wave", N, 70, 71, 301),            # waves 1 and 2
    ("scn", "wave_3_then_wave_0", N, 4, 5, 302),        # the lower row in wave 3 (k = 0), the higher in wave 0 (k = 1)
    ("scn", "across_slabs", N, 70, 134, 303),           # slabs 1 and 2
    ("scn", "gemm_tile_edge", N, 128, 129, 304),
]
TIE_TEMP = 0.1


def tie_id(c):
    return "%s-%s" % (c[0], c[1])


def tie_inputs(c, seed=3):
    """one proposal of matched pairs; row `second` of the template (scene) cloud is assigned from row `first`, and row `where` of the
    other cloud is a noisy copy of it -> F (2, n, 256), pts2 (1, n-1, 3)"""
    axis, _, n, first, second, where = c
    scn, tpl, pts2 = proposal("plain", n, seed + TIE_CASES.index(c))
    g = gen(9000 + TIE_CASES.index(c))
    if axis == "tpl":
        tpl[second] = tpl[first]
        scn[where] = tpl[first] + 0.25 * torch.randn(C, generator=g)
    else:
        scn[second] = scn[first]
        tpl[where] = scn[first] + 0.25 * torch.randn(C, generator=g)
    return stack([(scn, tpl, pts2)])


# ------------------------------------------------------------------------------------------------------------------ split entry
def split_inputs(B, n, scale, seed=0):
    """x (2B n, 256) tokens whose projection is a set of matched pairs, a random 256 -> 256 out_proj (W, b); x and b carry `scale`,
    which the normalisation removes"""
    g = gen(11000 + 7 * B + n + seed)
    W = (torch.rand(C, C, generator=g) * 2 - 1) / 16
    b = (torch.rand(C, generator=g) * 2 - 1) / 16 * scale
    tpl = torch.randn(B, n, C, generator=g)
    scn = torch.stack([tpl[i][torch.randperm(n, generator=g)] for i in range(B)]) + 0.25 * torch.randn(B, n, C, generator=g)
    x = (torch.cat([scn, tpl]).reshape(2 * B * n, C) * scale).contiguous()
    pts2 = (torch.rand(B, n - 1, 3, generator=g) - 0.5).contiguous()
    return x, W, b, pts2


def best_exponent64(F, B, temp):
    """the largest exponent (cos - 1) log2e / temp of every row of the fixed-shift E, in float64 -> (B, n)"""
    return torch.stack([(att64(F, b, B, 1.0).max(1).values - 1.0) * (LOG2E / temp) for b in range(B)])


def min_cos64(F, B):
    return min(float(att64(F, b, B, 1.0).min()) for b in range(B))
