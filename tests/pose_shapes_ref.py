"""Float64 restatements of the pose-solver operations (what csrc/pose.hip computes: PEM/utils/model_utils.py:204-436), the seeded
input builders of tests/test_pose_shapes_gpu.py / tests/test_pose_shapes_host.py, the conditions under which index outputs are compared
exactly, and the table of bounds.  Plain torch on the CPU; no GPU, no product code.  The 3 x 3 solves are torch.linalg.svd in float64.

An arg-max is only comparable between two precisions when the high-precision values clear the decision: `soft_assign64` marks the rows
and columns whose two best float64 values lie within LABEL_REL of each other (left out, at most LABEL_SHARE of a shape), `score_case`
re-draws its poses until the two best float64 scores differ by twice SCORE_GAP, and the Procrustes builders re-draw until the cut
share, the distance of every weight from the threshold and the conditioning hold.  The re-draws are part of the seeded construction;
the host test asserts every condition."""
import functools
import math

import torch

LABEL_REL = 1e-5    # float64 top two of a row / column of S closer than this (relative): label left out (the hardware exp / rcp is ~1e-6 a factor)
LABEL_SHARE = 0.01  # largest share of a shape's rows, and of its columns, that may be left out
SCORE_GAP = 1e-3    # relative gap of the float64 top two hypothesis scores above which `best` is compared
MIN_DIST = 0.2      # smallest nearest-CAD-point distance of the scoring scenes
SIGMA_RATIO = 0.05  # the suite's conditioning filter of 3-point problems (tests/test_pem_gpu.py): sigma2 / sigma1 of the correlation matrix
W_THRESH = 0.3      # weight_thresh of the cut Procrustes cases
W_CLEAR = 1e-6      # distance every weight keeps from W_THRESH

# Every bound is one the suite already holds these quantities to, or is derived in the function named:
TOL = dict(
    assign=1e-5,        # weights, w1, weight, pred: tests/test_configs_gpu.py::test_fine_stage_labels_and_weights_vs_oracle (max abs)
    hyp_Rt=1e-4,        # well-posed 3-point R, t: test_coarse_rt_flat_attention (max abs)
    hyp_dis=2e-6,       # hypothesis residuals: the same test
    proper=1e-5,        # orthonormality / determinant of a returned rotation: test_procrustes_golden
    score_rel=1e-4,     # hypothesis scores vs float64, relative: test_coarse_rt_flat_attention
    routes_rel=2e-6,    # matrix-core vs vector-ALU scores, relative: test_coarse_rt_large_model_cloud
    proc_R=2e-5,        # N-point weighted R: test_procrustes_golden (weighted case)
    proc_t=5e-4,        # N-point t: test_procrustes_golden
    dir2=1e-5,          # N = 2: R maps the centred source direction onto the centred reference direction
    coarse_Rt=1e-4,     # compute_coarse_Rt pose: test_coarse_rt_large_model_cloud
)


def sum_tol(n):
    """relative bound of an fp32 sum of n positive terms exp(a - max) against float64: any summation order is within (n - 1) * 2^-24,
    expf adds about 2^-23 per term -> (n + 4) * 2^-24"""
    return (n + 4) * 2.0 ** -24


def gen(seed):
    return torch.Generator().manual_seed(seed)


def first_argmax(x, dim):
    """index of the FIRST maximum along dim"""
    n = x.shape[dim]
    shape = [1] * x.dim()
    shape[dim] = n
    idx = torch.arange(n).reshape(shape).expand_as(x)
    return torch.where(x == x.max(dim, keepdim=True).values, idx, torch.full_like(idx, n)).min(dim).values


def random_rotations(n, g):
    q = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64)).Q
    q[:, :, 0] *= torch.sign(torch.linalg.det(q))[:, None]
    return q.float().contiguous()


def proper_error(R):
    """largest of |R R^T - I| and |det R - 1| over a stack of 3 x 3 matrices"""
    R = R.double().reshape(-1, 3, 3)
    return max(float((R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()), float((torch.linalg.det(R) - 1).abs().max()))


# ------------------------------------------------------------------------------------------------------- soft assignment
# (R, C): both sides of R = 256 (one row slice / 16 slices, expf / hardware exp) and of C = 2304 (register-resident row / loop),
# C < 64, (R-1) % 4 != 0 (four rows share a workgroup), C % 256 != 0, R = 257 (16 slices of 17 rows: the last holds 2)
SA_SHAPES = [(2, 2), (3, 70), (65, 64), (197, 197), (256, 300), (257, 300), (258, 257), (300, 2304), (260, 2305), (5, 2305), (2049, 130)]
SA_B = 2
SA_SLICES = 16
TIE_SHAPES = [(197, 197), (257, 300), (260, 2305)]
TIE_KINDS = ("col_same_lane", "col_other_lane", "row_in_slice", "row_across_slices")
ASSIGN_SHAPES = [(65, 64), (256, 300), (257, 300), (260, 2305)]
BG_ROW = 3  # the row of the assignment cases whose label is the bg column


def sa_id(s):
    return "x".join(map(str, s))


def slice_rows(R):
    """the rows at which sam6d_soft_assign cuts the matrix: the last row of every slice and the first row of the next"""
    if R <= 256:
        return []
    per = (R + SA_SLICES - 1) // SA_SLICES
    return [r for s in range(1, SA_SLICES) for r in (s * per - 1, s * per) if r < R]


def sa_inputs(R, C, B=SA_B, seed=0):
    """randn * 3, then one entry per row and one per column raised by 6 at the places where a tail goes wrong: rows get theirs in the
    last column or in column 63 / 64 / 255 / 256 / 2303 / 2304 (those that exist), columns get theirs in the last row or at a slice
    edge.  exp(6) = 400 against a row of ~exp(4.5) sum-exp per 100 entries: dropping or doubling that element moves the sum by tens
    of percent."""
    g = gen(100 + seed + 7 * R + C)
    att = torch.randn(B, R, C, generator=g) * 3
    cols = [c for c in (C - 1, 63, 64, 255, 256, 2303, 2304) if 0 <= c < C]
    rows = [R - 1] + slice_rows(R)
    for r in range(R):
        att[:, r, cols[r % len(cols)]] += 6.0
    for c in range(C):
        att[:, rows[c % len(rows)], c] += 6.0
    return att.contiguous()


def soft_assign64(att):
    """PEM/utils/model_utils.py:229-232 (= :320-322) in float64 -> dict: rmax / cmax (fp32 maxima: a max rounds nothing), rsum / csum
    (float64 sum exp(a - max)), S (B,R,C) f64, l1 (B,R-1) / l2 (B,C-1) first arg-max, near1 / near2: labels left out by LABEL_REL"""
    a = att.double()
    rmax, cmax = att.max(2).values, att.max(1).values
    er, ec = torch.exp(a - rmax.double()[:, :, None]), torch.exp(a - cmax.double()[:, None, :])
    rsum, csum = er.sum(2), ec.sum(1)
    S = (er / rsum[:, :, None]) * (ec / csum[:, None, :])  # softmax(dim=2) * softmax(dim=1)
    S1, S2 = S[:, 1:, :], S[:, :, 1:]
    l1, l2 = first_argmax(S1, 2), first_argmax(S2, 1)

    def near(x, dim):
        if x.shape[dim] < 2:
            return torch.zeros_like(x.select(dim, 0), dtype=torch.bool)
        top = torch.topk(x, 2, dim=dim).values
        t0, t1 = top.select(dim, 0), top.select(dim, 1)
        return (t0 - t1) <= LABEL_REL * t0

    return dict(rmax=rmax, cmax=cmax, rsum=rsum, csum=csum, S=S, l1=l1, l2=l2, near1=near(S1, 2), near2=near(S2, 1))


@functools.lru_cache(maxsize=None)
def sa_case(R, C):
    """(att, soft_assign64(att)) of one SA_SHAPES entry, built once per process and left unchanged"""
    att = sa_inputs(R, C)
    return att, soft_assign64(att)


def tie_places(R, C, kind):
    """(first, second) index of the duplicated column / row of a tie case, or None where the shape has no such case"""
    per = (R + SA_SLICES - 1) // SA_SLICES
    if kind == "col_same_lane":
        return (C - 66, C - 2)           # 64 apart: one lane of the row pass holds both; the copy sits in the row's tail
    if kind == "col_other_lane":
        return (5, C - 1)                # the copy is the last column
    if kind == "row_in_slice":
        return (per + 2, per + 7) if R > 256 else (20, 25)
    if kind == "row_across_slices":
        return (per + 2, R - 1) if R > 256 else None   # the copy is the last row, in the last slice
    raise KeyError(kind)


TIE_CASES = [(R, C, kind) for (R, C) in TIE_SHAPES for kind in TIE_KINDS if tie_places(R, C, kind) is not None]  # (no pair of rows in two slices at R <= 256)


def tie_id(c):
    return "%dx%d-%s" % c


def tie_inputs(R, C, kind, B=SA_B, seed=0):
    """sa_inputs with column c1 (row r1) set to 30 .. 31 in eleven rows (columns) -- it becomes their maximum of S by a wide margin --
    and then copied bitwise to c2 (r2).  -> att, dict(axis, first, second, where): `where` are the rows (columns) whose label is the tied pair."""
    first, second = tie_places(R, C, kind)
    att = sa_inputs(R, C, B, seed + 17)
    g = gen(900 + seed + R + C + TIE_KINDS.index(kind))
    if kind.startswith("col"):
        where = (torch.randperm(R - 1, generator=g)[:11] + 1).sort().values
        att[:, where, first] = 30.0 + torch.rand(B, 11, generator=g)
        att[:, :, second] = att[:, :, first]
    else:
        where = torch.tensor([c for c in (torch.randperm(C - 1, generator=g)[:11] + 1).sort().values.tolist()])
        att[:, first, where] = 30.0 + torch.rand(B, 11, generator=g)
        att[:, second, :] = att[:, first, :]
    return att.contiguous(), dict(axis="col" if kind.startswith("col") else "row", first=first, second=second, where=where)


def bg_inputs(R, C, B=SA_B, seed=0):
    """the bg column wins every second row and the bg row every second column: labels 0 and above 0 both occur"""
    att = sa_inputs(R, C, B, seed + 29)
    g = gen(1100 + seed + R + C)
    att[:, 1::2, 0] = 25.0 + torch.rand(B, len(range(1, R, 2)), generator=g)
    att[:, 0, 1::2] = 25.0 + torch.rand(B, len(range(1, C, 2)), generator=g)
    return att.contiguous()


def assign_inputs(R, C, B=SA_B, seed=0):
    """-> att (row BG_ROW prefers the bg column by 30: its label is 0), pts2 (B,C-1,3) in [-0.5, 0.5]"""
    att = sa_inputs(R, C, B, seed + 41)
    att[:, BG_ROW, 0] += 30.0
    g = gen(1300 + seed + R + C)
    return att.contiguous(), (torch.rand(B, C - 1, 3, generator=g) - 0.5).contiguous()


def assign64(att, l1, l2, pts2):
    """PEM/utils/model_utils.py:233-238 and :324-330 in float64 from GIVEN labels (the caller passes the labels of the implementation
    under test, so that a left-out near-tie does not propagate) -> weights (B,(R-1)(C-1)), w1 (B,R-1), weight (B,R-1), pred (B,R-1,3)"""
    S = soft_assign64(att)["S"]
    w1, w2 = (l1 > 0).double(), (l2 > 0).double()
    A = S[:, 1:, 1:] * w1[:, :, None] * w2[:, None, :]
    weight = A.sum(2)
    pred = (A / (weight[:, :, None] + 1e-6)) @ pts2.double()
    return dict(weights=A.reshape(A.shape[0], -1) ** 1.5, w1=w1, weight=weight, pred=pred)


# ------------------------------------------------------------------------------------------- one-launch coarse path (LDS bound)
def cas_lds_bytes(R, C):
    """dynamic LDS of sam6d_coarse_soft_assign: the matrix, two statistics and a label per row and per column"""
    return (R * C + 3 * R + 3 * C) * 4


CAS_LIMIT = 160 * 1024
# (B, R, C): the largest square, a wide shape EXACTLY at the bound, a tall one just inside it (R = 256: the tallest whose two-call form
# still sums a column in one slice), C < 64
CAS_SHAPES = [(3, 199, 199), (2, 50, 770), (2, 256, 155), (2, 200, 40)]
CAS_OVER = (200, 200)  # the first square over the bound


def coarse_scene(gold, n=199, seed=0):
    """The known-answer scene of tests/golden/coarse_rt.npz (196 template points, the scene points their permuted images under the
    ground-truth pose) extended to n points a side with seeded random template points and their images; the attention is the golden
    scene's recipe on the extended clouds: clamp(1 - 4 d, -1) / 0.1 between the scene points in the template frame and the template
    points, bg row / column -10.  -> att (B,n+1,n+1), p1, p2 (B,n,3), model (B,1024,3), u (B,18000)"""
    g = gen(1700 + seed + n)
    p1, p2, model, u, Rg, tg = (torch.from_numpy(gold[k]).float() for k in ("p1", "p2", "model", "u", "R_gt", "t_gt"))
    B = p1.shape[0]
    e2 = torch.rand(B, n - p2.shape[1], 3, generator=g) - 0.5
    p2x = torch.cat([p2, e2], 1).contiguous()
    p1x = torch.cat([p1, e2 @ Rg.transpose(1, 2) + tg[:, None, :]], 1).contiguous()
    d = torch.cdist((p1x - tg[:, None, :]) @ Rg, p2x)
    att = torch.full((B, n + 1, n + 1), -10.0)
    att[:, 1:, 1:] = torch.clamp(1 - 4.0 * d, min=-1) / 0.1
    return att.contiguous(), p1x, p2x, model.contiguous(), u.contiguous()


# ------------------------------------------------------------------------------------------------------- 3-point hypotheses
HYP = dict(B=3, N1=50, N2=119, nh=257)  # N1 != N2: idx / N2 and idx % N2; B * nh = 771 = 3 * 256 + 3
HYP_DEGENERATE = ("pair_twice", "pair_three_times", "collinear", "both_sides")


def hyp_inputs(seed=0):
    """-> pts1 (B,N1,3) scene, pts2 (B,N2,3) template, idx (B,3*nh) i32 uniform in [0, N1*N2), deg (B,12) i32: the four hand-built
    degenerate hypotheses of HYP_DEGENERATE.  Points 0, 1, 2 of both clouds are collinear."""
    B, N1, N2, nh = (HYP[k] for k in ("B", "N1", "N2", "nh"))
    g = gen(2100 + seed)
    pts1 = torch.rand(B, N1, 3, generator=g) - 0.5
    pts2 = torch.rand(B, N2, 3, generator=g) - 0.5
    pts1[:, 2] = pts1[:, 0] + 1.75 * (pts1[:, 1] - pts1[:, 0])
    pts2[:, 2] = pts2[:, 0] - 0.5 * (pts2[:, 1] - pts2[:, 0])
    idx = torch.randint(0, N1 * N2, (B, 3 * nh), generator=g).to(torch.int32)
    pair = lambda a, c: a * N2 + c
    deg = torch.tensor([pair(7, 11), pair(7, 11), pair(30, 100),       # a pair repeated twice
                        pair(49, 118), pair(49, 118), pair(49, 118),  # a pair repeated three times (the last points of both clouds)
                        pair(0, 20), pair(1, 40), pair(2, 60),        # three collinear scene points
                        pair(0, 0), pair(1, 1), pair(2, 2)],          # collinear on both sides
                       dtype=torch.int32).repeat(B, 1)
    return pts1.contiguous(), pts2.contiguous(), idx.contiguous(), deg.contiguous()


def hyp_triples(idx, pts1, pts2, nh):
    """PEM/utils/model_utils.py:249-254 -> p1, p2 (B,nh,3,3) f64, i1, i2 (B,nh,3)"""
    B, N1, _ = pts1.shape
    N2 = pts2.shape[1]
    idx = idx.long()
    i1 = torch.clamp(idx.div(N2, rounding_mode="floor"), max=N1 - 1)
    i2 = torch.clamp(idx % N2, max=N2 - 1)
    p1 = torch.gather(pts1.double(), 1, i1[:, :, None].expand(B, 3 * nh, 3)).reshape(B, nh, 3, 3)
    p2 = torch.gather(pts2.double(), 1, i2[:, :, None].expand(B, 3 * nh, 3)).reshape(B, nh, 3, 3)
    return p1, p2, i1.reshape(B, nh, 3), i2.reshape(B, nh, 3)


def kabsch64(H):
    """PEM/utils/model_utils.py:404-420: R = V diag(1, 1, sign det(V U^T)) U^T of H = U S V^T, torch.linalg.svd in float64"""
    U, _, Vh = torch.linalg.svd(H)
    V, Ut = Vh.transpose(-1, -2), U.transpose(-1, -2)
    D = torch.eye(3, dtype=torch.float64).expand_as(H).clone()
    D[..., 2, 2] = torch.sign(torch.linalg.det(V @ Ut))
    return V @ D @ Ut


def procrustes64(src, ref, weights=None, weight_thresh=0.0, eps=1e-5):
    """PEM/utils/model_utils.py:343-436 in float64: src, ref (...,N,3), weights (...,N) -> R (...,3,3), t (...,3), H"""
    src, ref = src.double(), ref.double()
    w = torch.ones_like(src[..., 0]) if weights is None else weights.double()
    w = torch.where(w < weight_thresh, torch.zeros_like(w), w)                                   # :382
    w = (w / (w.sum(-1, keepdim=True) + eps))[..., None]                                          # :383-384
    sc, rc = (src * w).sum(-2, keepdim=True), (ref * w).sum(-2, keepdim=True)                     # :387, :393
    H = (src - sc).transpose(-1, -2) @ (w * (ref - rc))                                           # :398
    R = kabsch64(H)
    t = (rc.transpose(-1, -2) - R @ sc.transpose(-1, -2))[..., 0]                                 # :422
    return R, t, H


def hypotheses64(idx, pts1, pts2, nh):
    """PEM/utils/model_utils.py:249-261: R, t = procrustes(p2 triple -> p1 triple) with unit weights (1 / (3 + 1e-5) after the
    normalisation), dis = mean_k |(p1_k - t) R - p2_k|.  -> Rs (B,nh,3,3), ts (B,nh,3), dis (B,nh), wellposed (B,nh) bool: distinct
    points on both sides and sigma2 / sigma1 > SIGMA_RATIO"""
    p1, p2, i1, i2 = hyp_triples(idx, pts1, pts2, nh)
    Rs, ts, H = procrustes64(p2, p1, None, 0.5)
    dis = residual64(p1, p2, Rs, ts)
    distinct = lambda x: (x[..., 0] != x[..., 1]) & (x[..., 0] != x[..., 2]) & (x[..., 1] != x[..., 2])
    sv = torch.linalg.svdvals(H)
    well = distinct(i1) & distinct(i2) & (sv[..., 1] / sv[..., 0].clamp_min(1e-300) > SIGMA_RATIO)
    return Rs, ts, dis, well


def residual64(p1, p2, Rs, ts):
    """PEM/utils/model_utils.py:261 from GIVEN poses: mean_k |(p1_k - t) R - p2_k|"""
    return torch.linalg.norm((p1 - ts.double()[..., None, :]) @ Rs.double() - p2, dim=-1).mean(-1)


# ------------------------------------------------------------------------------------------------------- hypothesis scoring
SCORE_NH = 400
# (N1, k, P): the product {1, 37, 196, 257} x {1, 5, 63, 300} x {1, 31, 33, 1000} thinned so that every value occurs at least twice.
# k * N1 % 32 != 0 in most, k % 4 in {1, 3, 0} (the groups of four clamp to k - 1), k < 64 and k > 64 (pick_best), P % 32 and P % 4 tails
SCORE_CASES = [(1, 1, 1), (1, 63, 1000), (1, 300, 33), (37, 1, 31), (37, 5, 31), (37, 63, 1000), (196, 1, 33), (196, 5, 1),
               (196, 300, 1000), (257, 5, 33), (257, 63, 31), (257, 300, 1)]
SCORE_VECTOR_ONLY = [(37, 5, 4097), (37, 5, 8192)]  # beyond the matrix-core route: 64 KB + 16 B and 128 KB of CAD points in LDS
SCORE_TIE = (196, 300, 33)


def score64(sel, Rs, ts, pts1, w1, model, radius):
    """PEM/utils/model_utils.py:263-272 in float64 (model / (radius + 1e-6): PEM/model/coarse_point_matching.py:60) ->
    scores (B,k), dmin: the smallest nearest-CAD-point distance, best (B,) = sel[first arg-max], gap (B,): relative gap of the top two"""
    B, k = sel.shape
    m = model.double() / (radius.double().reshape(B, 1, 1) + 1e-6)
    scores = torch.empty(B, k, dtype=torch.float64)
    dmin = math.inf
    w = w1.double()
    for b in range(B):
        R = Rs[b, sel[b].long()].double().reshape(k, 3, 3)
        t = ts[b, sel[b].long()].double().reshape(k, 1, 3)
        for s0 in range(0, k, 32):
            x = (pts1[b].double()[None] - t[s0:s0 + 32]) @ R[s0:s0 + 32]                      # :267
            d = torch.cdist(x, m[b][None].expand(x.shape[0], -1, -1),
                            compute_mode="donot_use_mm_for_euclid_dist").min(2).values       # :269-270 (differences, not |x|^2 - 2xy + |y|^2)
            dmin = min(dmin, float(d.min()))
            scores[b, s0:s0 + 32] = w[b].sum() / ((d * w[b]).sum(1) + 1e-8)                  # :271
    first = first_argmax(scores, 1)
    best = sel.long().gather(1, first[:, None])[:, 0]
    if k > 1:
        top = torch.topk(scores, 2, dim=1).values
        gap = (top[:, 0] - top[:, 1]) / top[:, 0].clamp_min(1e-300)
    else:
        gap = torch.full((B,), math.inf, dtype=torch.float64)
    return dict(scores=scores, dmin=dmin, best=best, first=first, gap=gap)


def _score_draw(N1, k, P, B, g, w1_kind):
    nh = SCORE_NH
    # CAD points within 0.3 of the origin (a cluster of radius 0.12 around a point 0.18 out), scene points in the shell 0.6 .. 0.9 (a
    # cap around one direction, so that a rotation moves the whole cloud towards or away from the CAD cluster and the scores spread),
    # |t| <= 0.05: every posed scene point has norm 0.55 .. 0.95 -- inside the unit ball, at least 0.25 from every CAD point
    radius = 0.5 + torch.rand(B, generator=g)
    unit = lambda x: x / x.norm(dim=-1, keepdim=True)
    m = 0.18 * unit(torch.randn(B, 1, 3, generator=g)) + unit(torch.randn(B, P, 3, generator=g)) * (0.12 * torch.rand(B, P, 1, generator=g) ** (1 / 3))
    model = (m * (radius.reshape(B, 1, 1) + 1e-6)).contiguous()
    cap = unit(unit(torch.randn(B, 1, 3, generator=g)) + 0.5 * torch.randn(B, N1, 3, generator=g))
    pts1 = (cap * (0.6 + 0.3 * torch.rand(B, N1, 1, generator=g))).contiguous()
    Rs = random_rotations(B * nh, g).reshape(B, nh, 9).contiguous()
    ts = (unit(torch.randn(B, nh, 3, generator=g)) * (0.05 * torch.rand(B, nh, 1, generator=g))).contiguous()
    sel = torch.stack([torch.randperm(nh, generator=g)[:k] for _ in range(B)]).to(torch.int32).contiguous()
    if w1_kind == "ones":
        w1 = torch.ones(B, N1)
    elif w1_kind == "zero":
        w1 = torch.zeros(B, N1)
    else:
        w1 = (torch.rand(B, N1, generator=g) > 0.3).float()
        w1[:, 0] = 1.0
    return dict(sel=sel, Rs=Rs, ts=ts, pts1=pts1, w1=w1.contiguous(), model=model, radius=radius.contiguous(), nh=nh, N1=N1, k=k, P=P, B=B)


@functools.lru_cache(maxsize=None)
def score_case(N1, k, P, w1_kind="mixed", tie=False, B=2, seed=0):
    """Seeded scene of one scoring case with its float64 result under "want"; drawn again (at most 20 times) until the float64 top two
    scores of every batch element differ by 2 * SCORE_GAP.  w1_kind: "mixed" (zeros and ones), "ones", "zero" (every score is 0).
    tie: the best hypothesis is copied bitwise into a second slot of `sel`, in another position of its group of four."""
    g = gen(3100 + seed + 1000 * N1 + 10 * k + P)
    d = _score_draw(N1, k, P, B, g, w1_kind)
    for _ in range(50):
        want = score64(d["sel"], d["Rs"], d["ts"], d["pts1"], d["w1"], d["model"], d["radius"])
        bad = want["gap"] <= 2 * SCORE_GAP
        if w1_kind == "zero" or not bad.any():
            break
        fresh = _score_draw(N1, k, P, B, g, w1_kind)  # the batch elements that miss the gap are drawn again
        for key in ("sel", "Rs", "ts", "pts1", "w1", "model", "radius"):
            d[key][bad] = fresh[key][bad]
    if tie:
        for b in range(B):
            a = int(want["first"][b])
            o = (a + 5) % k if (a + 5) % k != a else (a + 1) % k   # another slot: 5 further on, so another position in its group
            src, dst = int(d["sel"][b, a]), int(d["sel"][b, o])
            d["Rs"][b, dst] = d["Rs"][b, src]
            d["ts"][b, dst] = d["ts"][b, src]
        want = score64(d["sel"], d["Rs"], d["ts"], d["pts1"], d["w1"], d["model"], d["radius"])
    d["want"] = want
    return d


def score_second_gap(scores, exclude_equal=True):
    """relative gap between the maximum and the largest value below it (the exact copies of the maximum left out), per batch element"""
    top = scores.max(1, keepdim=True).values
    below = torch.where(scores < top, scores, torch.full_like(scores, -math.inf)).max(1).values
    return (top[:, 0] - below) / top[:, 0]


# ------------------------------------------------------------------------------------------------------- N-point Procrustes
# N <= 2048 keeps the points in registers, longer clouds are re-read (2049, 4097); N < 256: threads without a point; 255 / 256 / 257
PROC_N = (1, 2, 3, 4, 255, 256, 257, 2047, 2048, 2049, 4097)
PROC_MODES = ("none", "rand", "cut")
PROC_B = 3


def proc_conditioning(H):
    """(sigma2 - sigma3) / sigma1 of the correlation matrix: the suite's filter of test_procrustes_golden (> SIGMA_RATIO: R is well defined)"""
    sv = torch.linalg.svdvals(H)
    return (sv[..., 1] - sv[..., 2]) / sv[..., 0].clamp_min(1e-300)


@functools.lru_cache(maxsize=None)
def proc_case(N, mode, B=PROC_B, seed=0):
    """src (B,N,3) randn, ref = src Rgt^T + tgt + 1e-3 randn, weights None / rand / rand cut at W_THRESH -> dict with the float64 result
    (R, t, H, cond).  Drawn again until: ("cut") between 20 % and 40 % of the B * N weights lie below the threshold and none within
    W_CLEAR of it; (N >= 4) every problem passes the conditioning filter."""
    g = gen(4100 + seed + 13 * N + PROC_MODES.index(mode))
    for _ in range(200):
        src = torch.randn(B, N, 3, generator=g)
        Rgt = random_rotations(B, g)
        tgt = torch.randn(B, 1, 3, generator=g)
        ref = src @ Rgt.transpose(1, 2) + tgt + 1e-3 * torch.randn(B, N, 3, generator=g)
        w = None if mode == "none" else torch.rand(B, N, generator=g)
        thresh = W_THRESH if mode == "cut" else 0.0
        R, t, H = procrustes64(src, ref, w, thresh)
        cond = proc_conditioning(H)
        ok = True
        if mode == "cut":
            share = float((w < W_THRESH).float().mean())
            ok = 0.2 <= share <= 0.4 and float((w.double() - W_THRESH).abs().min()) > W_CLEAR
        if N >= 4:
            ok = ok and bool((cond > SIGMA_RATIO).all())
        if ok:
            break
    return dict(src=src.contiguous(), ref=ref.contiguous(), w=None if w is None else w.contiguous(), thresh=thresh, R=R, t=t, H=H, cond=cond,
                kept=None if w is None else (w >= thresh))


def direction_error(R, src, ref, w):
    """N = 2: |R d_src - d_ref| with d the unit vector from point 0 to point 1 (the centred points of a two-point cloud are parallel to
    it whatever the weights)"""
    ds = (src[:, 1] - src[:, 0]).double()
    dr = (ref[:, 1] - ref[:, 0]).double()
    ds, dr = ds / ds.norm(dim=-1, keepdim=True), dr / dr.norm(dim=-1, keepdim=True)
    return ((R.double() @ ds[:, :, None])[:, :, 0] - dr).abs().amax(-1)


# ------------------------------------------------------------------------------------------------------- fine pose score
# (N, P, thr): P = 31 / 33 / 97 (the +inf padding of the matrix-core planes to 32 rows, one and several row tiles; the tail of the vector
# minimum), N = 63 / 65 / 300 (a wave's column tiles and the vector kernel's 64 points on both sides of a workgroup, several workgroups),
# P = 3264 the last cloud on the matrix cores and P = 3265 the first on the vector ALU
FINE_SCORE_CASES = [(63, 31, 0.3), (65, 33, 0.3), (300, 97, 0.2), (257, 3264, 0.05), (257, 3265, 0.05)]
FINE_SCORE_SWITCH = (257, 3264, 0.05)  # the cloud that gets one duplicate point to cross the route switch
FINE_SCORE_RADIUS = (1.0, 0.5)
FINE_SCORE_GAP = 1e-5  # every float64 nearest distance stays this far from thr; the fp32 recipe errs by ~1e-7 / (2 d) = 2e-6 at d = 0.05


def fine_score64(p1, R, t, model, radius, l1, thr):
    """PEM/utils/model_utils.py:331-339 in float64 (model / (radius + 1e-6): PEM/model/fine_point_matching.py) -> near (B,), mask (B,)
    counts, score (B,), gap: the smallest |nearest distance - thr|"""
    m = model.double() / (radius.double().reshape(-1, 1, 1) + 1e-6)
    x = (p1.double() - t.double()[:, None, :]) @ R.double()
    d = torch.cdist(x, m, compute_mode="donot_use_mm_for_euclid_dist").min(2).values
    mask = l1.double()
    near, mk = ((d < thr).double() * mask).sum(1), mask.sum(1)
    return dict(near=near, mask=mk, score=near / (mk + 1e-8) * mask.mean(1), gap=float((d - thr).abs().min()))


@functools.lru_cache(maxsize=None)
def fine_score_case(N, P, thr, B=2):
    """seeded scene of one sam6d_fine_score case with its float64 counts under "want"; the draws come from one generator in this order"""
    g = gen(1000 * N + P)
    p1 = torch.rand(B, N, 3, generator=g) - 0.5
    model = torch.rand(B, P, 3, generator=g) - 0.5
    R = torch.linalg.qr(torch.randn(B, 3, 3, generator=g)).Q.contiguous()
    t = (torch.rand(B, 3, generator=g) - 0.5) * 0.1
    l1 = (torch.rand(B, N, generator=g) > 0.3).to(torch.int32)
    radius = torch.tensor(FINE_SCORE_RADIUS)
    d = dict(p1=p1.contiguous(), model=model.contiguous(), R=R, t=t.contiguous(), l1=l1.contiguous(), radius=radius, thr=thr, B=B, N=N, P=P)
    d["want"] = fine_score64(p1, R, t, model, radius, l1, thr)
    return d
