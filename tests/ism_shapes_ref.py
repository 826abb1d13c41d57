"""Float64 restatements of the ISM template-scoring operations (what csrc/ism.hip computes), the seeded input builders of
tests/test_ism_shapes_gpu.py / tests/test_ism_shapes_host.py, and the input conditions under which index and count outputs are
compared exactly.  Plain torch on the CPU; no GPU, no reference code.

An index or a thresholded count is only comparable between two precisions when the high-precision value clears the decision:
every builder below repairs its draw until the float64 value is at least MARGIN away from each decision it feeds (the repairs are
part of the seeded construction), and the `*_conditions` functions return the measured margins for the tests to assert.
"""
import functools
import math

import torch

MARGIN = 1e-5     # distance a float64 value keeps from a threshold / a competing value
PX_MARGIN = 1e-3  # distance (pixels) a float64 projection keeps from an integer for its truncation to be compared
PX_SHARE = 1e-3   # largest share of projected coordinates that may be left out by PX_MARGIN
TOL = dict(sim=2e-6, sem=2e-6, appe=5e-6, vis=2e-6, iou=1e-6, final=5e-6)  # what the golden fixture holds these quantities to
CAM_K = [572.4114, 0.0, 325.2611, 0.0, 573.57043, 242.04899, 0.0, 0.0, 1.0]  # the demo camera of the 480 x 640 fixture


def gen(seed):
    return torch.Generator().manual_seed(seed)


def first_argmax(x):
    """index of the FIRST maximum along the last dimension"""
    n = x.shape[-1]
    idx = torch.arange(n).expand_as(x)
    return torch.where(x == x.max(-1, keepdim=True).values, idx, torch.full_like(idx, n)).min(-1).values


# ------------------------------------------------------------------------------------------------------------- cosine
COSINE_SHAPES = [(1, 1, 1, 4), (7, 3, 5, 36), (5, 1, 3, 260), (33, 2, 162, 1024), (200, 8, 42, 1024)]  # (Nq, No, Nt, D)


def cosine_inputs(Nq, No, Nt, D, seed=0):
    g = gen(1000 + seed + Nq + 7 * Nt + D)
    return torch.randn(Nq, D, generator=g), torch.randn(No, Nt, D, generator=g)


def cosine_edge_inputs(D=36, seed=0):
    """query rows: 0 all-zero, 1 = template (0,1) (clamps at 1), 2 = -template (0,2) (clamps at 0), 3 scaled by 1e15, 4 by 1e-15,
    5 plain; template (0,0) all-zero, (1,0) scaled by 1e15, (1,1) by 1e-15.  Returns q (6,D), ref (2,3,D)."""
    g = gen(1100 + seed + D)
    q, ref = torch.randn(6, D, generator=g), torch.randn(2, 3, D, generator=g)
    ref[0, 0] = 0
    ref[1, 0] *= 1e15
    ref[1, 1] *= 1e-15
    q[0] = 0
    q[1] = ref[0, 1]
    q[2] = -ref[0, 2]
    q[3] *= 1e15
    q[4] *= 1e-15
    return q, ref


def cosine64(query, reference):
    """F.normalize (eps 1e-12) on both sides, F.cosine_similarity (eps 1e-8), clamp to [0,1] -- in float64."""
    q, r = query.double(), reference.double()
    qn = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    rn = r / r.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    dot = torch.einsum("qd,otd->qot", qn, rn)
    den = qn.norm(dim=-1).clamp_min(1e-8)[:, None, None] * rn.norm(dim=-1).clamp_min(1e-8)[None]
    return (dot / den).clamp(0.0, 1.0)


# ------------------------------------------------------------------------------------------------------------- semantic
MODES = ("avg_5", "mean", "max")
SEM_NT = (1, 3, 4, 5, 6, 42, 64, 65, 128, 162, 255, 256)
SEM_NO = (1, 3, 8)
SEM_NQ = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 3072)


TIE_TEMPLATES = {"two": [5, 40], "same_lane": [5, 69, 133], "seven": [0, 3, 64, 67, 128, 129, 130]}  # tied templates at Nt = 162


def sem_cases():
    """(Nq, No, Nt, mode): every Nt with every No and mode at Nq = 65, every Nq with every mode at a small and at the largest (No, Nt)"""
    out = [(65, no, nt, m) for nt in SEM_NT for no in SEM_NO for m in MODES]
    out += [(nq, no, nt, m) for nq in SEM_NQ for (no, nt) in ((3, 65), (8, 256)) for m in MODES if nq != 65]
    return out


def aggregate64(scores, mode):
    """(Nq,No,Nt) -> (Nq,No) float64; avg_5 is the mean of the min(5, Nt) largest, equal values counted once each."""
    s = scores.double()
    if mode == "mean":
        return s.sum(-1) / s.shape[-1]
    if mode == "max":
        return s.max(-1).values
    if mode == "avg_5":
        k = min(5, s.shape[-1])
        return torch.topk(s, k, dim=-1).values.sum(-1) / k
    raise NotImplementedError(mode)


def semantic64(scores, mode, thresh):
    """-> dict: sem (Nq,) f64, obj (Nq,), best (Nq,) for EVERY query, sel = ascending indices with sem > thresh.
    First maximal object, first maximal template of that object."""
    s = scores.double()
    Nq, No, Nt = s.shape
    agg = aggregate64(s, mode)
    obj = first_argmax(agg) if Nq else torch.zeros(0, dtype=torch.int64)
    sem = agg.gather(1, obj[:, None])[:, 0] if Nq else torch.zeros(0, dtype=torch.float64)
    best = first_argmax(s[torch.arange(Nq), obj]) if Nq else torch.zeros(0, dtype=torch.int64)
    sel = torch.nonzero(sem > thresh)[:, 0]
    return dict(agg=agg, sem=sem, obj=obj, best=best, sel=sel)


def semantic_conditions(scores, mode, thresh, dup_obj=None):
    """(distance of the winning aggregate from the threshold, gap between the two best per-object aggregates), the smallest over the
    queries; dup_obj = (a, b): object b is an exact copy of object a and is left out of the gap."""
    agg = aggregate64(scores, mode)
    if agg.shape[0] == 0:
        return math.inf, math.inf
    if dup_obj is not None:
        agg = agg[:, [o for o in range(agg.shape[1]) if o != dup_obj[1]]]
    top = torch.topk(agg, min(2, agg.shape[1]), dim=-1).values
    gap = float((top[:, 0] - top[:, 1]).min()) if agg.shape[1] > 1 else math.inf
    return float((top[:, 0] - thresh).abs().min()), gap


def semantic_scores(Nq, No, Nt, mode, thresh=0.2, seed=0, low=False, dup_templates=None, dup_obj=None):
    """Seeded fp32 scores (Nq,No,Nt) in [0,1]: uniform draws times a per-(query, object) level in [0.1, 1], three queries in ten
    scaled down below the threshold, so that winners and the threshold decision vary; query 0 is won by object No-1 at template
    Nt-1.  Queries whose float64 aggregates miss a margin are drawn again.  low: every query scaled down (nothing passes 0.2).  dup_templates = [j0, j1, ...]: in every row those templates all hold the
    row's maximum (an exact tie at the top; j0 first).  dup_obj = (a, b): object b is a copy of object a and a wins every odd query."""
    g = gen(2000 + seed + 3 * Nq + 5 * No + 11 * Nt + MODES.index(mode))

    def draw(n):
        quiet = torch.rand(n, 1, 1, generator=g) < (2.0 if low else 0.3)  # these queries stay below the threshold whatever the mode
        lvl = (0.1 + 0.9 * torch.rand(n, No, 1, generator=g)) * torch.where(quiet, 0.15, 1.0)
        s = torch.rand(n, No, Nt, generator=g) * lvl
        if dup_templates:
            s[..., dup_templates] = s.max(-1, keepdim=True).values
        if dup_obj:
            a, b = dup_obj
            s[1::2, a] = (0.9 + 0.1 * torch.rand(n, Nt, generator=g))[1::2]
            s[:, b] = s[:, a]
        return s

    s = draw(Nq)
    planted = bool(Nq) and not low and not dup_templates and not dup_obj
    if planted:  # (clears every margin by construction: object No-1 at 0.6 .. 1, the others below 0.5)
        s[0] = s[0] * 0.5
        s[0, No - 1] = 0.6 + 0.3 * torch.rand(Nt, generator=g)
        s[0, No - 1, Nt - 1] = 1.0
    for _ in range(50):
        if Nq == 0:
            break
        agg = aggregate64(s, mode)
        if dup_obj:
            agg = agg[:, [o for o in range(No) if o != dup_obj[1]]]
        top = torch.topk(agg, min(2, agg.shape[1]), dim=-1).values
        bad = (top[:, 0] - thresh).abs() < 2 * MARGIN
        if agg.shape[1] > 1:
            bad |= (top[:, 0] - top[:, 1]) < 2 * MARGIN
        if planted:
            bad[0] = False
        if not bad.any():
            break
        s[bad] = draw(Nq)[bad]
    return s


def descriptor_inputs(Nq, No, Nt, D, mode="avg_5", thresh=0.2, seed=0):
    """Descriptors for compute_semantic_score end to end: three quarters of the queries resemble one object's templates, the rest are
    noise.  Queries whose float64 scores miss a margin (threshold, object gap, gap between the two best templates of the winning object)
    are drawn again."""
    g = gen(2500 + seed + Nq)
    base = torch.randn(No, 1, D, generator=g)
    ref = base + 0.7 * torch.randn(No, Nt, D, generator=g)

    def draw():
        q = torch.randn(Nq, D, generator=g)
        n = (3 * Nq) // 4
        q[:n] = base[torch.randint(0, No, (n,), generator=g), 0] + 0.8 * q[:n]
        return q

    q = draw()
    for _ in range(50):
        bad = torch.tensor(descriptor_margins(q, ref, mode, thresh, per_query=True)) < 2 * MARGIN
        if not bad.any():
            break
        q[bad] = draw()[bad]
    return q, ref


@functools.lru_cache(maxsize=None)
def descriptors_3072():
    return descriptor_inputs(3072, 3, 42, 64)


def descriptor_margins(q, ref, mode, thresh, per_query=False):
    s = cosine64(q, ref)
    r = semantic64(s, mode, thresh)
    top = torch.topk(r["agg"], min(2, r["agg"].shape[1]), dim=-1).values
    m = (top[:, 0] - thresh).abs()
    if top.shape[1] > 1:
        m = torch.minimum(m, top[:, 0] - top[:, 1])
    row = s[torch.arange(s.shape[0]), r["obj"]]
    if row.shape[1] > 1:
        t2 = torch.topk(row, 2, dim=-1).values
        m = torch.minimum(m, t2[:, 0] - t2[:, 1])
    return m.tolist() if per_query else float(m.min())


# ------------------------------------------------------------------------------------------------------------- patch scores
# (No, Nt, P, D, Ns); the second 512-patch case has room for all three special proposals of patch_roles
PATCH_SHAPES = [(3, 7, 128, 32, 5), (2, 5, 384, 64, 9), (4, 3, 512, 96, 3), (4, 3, 512, 96, 7), (8, 42, 256, 1024, 200)]
PATCH_THREDS = (0.5, 0.3, 0.7)


def _unit(x):
    return torch.nn.functional.normalize(x, dim=-1)


def patch_reduce64(q_appe, ref_appe, obj, best, q_index=None):
    """What both scores need of the (P,P) float64 similarity of every proposal with its template, one proposal at a time (the largest
    case is 200 products of 256 x 1024 x 256): dict of rowmax, colmax, rowsum (the query patches' coordinate sums) (Ns,P) f64 and
    live (Ns,P) bool (query patch not all-zero)."""
    out = dict(rowmax=[], colmax=[], rowsum=[], live=[])
    for p in range(obj.shape[0]):
        q = q_appe[int(q_index[p]) if q_index is not None else p].double()
        sim = q @ ref_appe[int(obj[p]), int(best[p])].double().T
        out["rowmax"].append(sim.max(1).values)
        out["colmax"].append(sim.max(0).values)
        out["rowsum"].append(q.sum(-1))
        out["live"].append((q != 0).any(-1))
    return {k: torch.stack(v) for k, v in out.items()}


def sim_reduce64(q_appe, sim):
    """the same from a given similarity tensor (Ns,P,P)"""
    s, q = sim.double(), q_appe.double()
    return dict(rowmax=s.max(2).values, colmax=s.max(1).values, rowsum=q.sum(-1), live=(q != 0).any(-1))


def patch_scores64(red, thred):
    """appearance = clamp(sum_rows max_cols sim / (count_nonzero(rowsum q) + 1e-6), 0, 1);
    visible = count(colmax > thred, colmax != 0) / (count_nonzero(colmax) + 1e-6)      -> (Ns,), (Ns,) float64"""
    appe = (red["rowmax"].sum(-1) / (torch.count_nonzero(red["rowsum"], dim=-1) + 1e-6)).clamp(0.0, 1.0)
    cm = red["colmax"]
    vis = torch.count_nonzero(cm * (cm > thred), dim=-1) / (torch.count_nonzero(cm, dim=-1) + 1e-6)
    return appe, vis


def patch_conditions(red, threds=PATCH_THREDS):
    """smallest distance of a column maximum from a threshold, of a non-zero column maximum from 0, and of the coordinate sum of a
    not-all-zero query patch from 0"""
    cm = red["colmax"]
    d_thr = min(float((cm - t).abs().min()) for t in threds)
    nz = cm[cm != 0]
    rs = red["rowsum"][red["live"]]
    return d_thr, (float(nz.abs().min()) if nz.numel() else math.inf), (float(rs.abs().min()) if rs.numel() else math.inf)


def patch_roles(Ns):
    """The special proposals of a patch case, taken from the end while two ordinary proposals remain: dict of proposal index or None.
    ng: the query patches are the negated patches of template (No-1, Nt-1), whose coordinates are all positive, so every similarity
    is negative (and a wrong stride, reading another slice, lifts the appearance off 0); zq: all-zero query patches; zt: the all-zero
    template (0, 0)."""
    return {name: (Ns - 1 - k if Ns - 1 - k >= 2 else None) for k, name in enumerate(("ng", "zq", "zt"))}


def patch_inputs(No, Nt, P, D, Ns, seed=0):
    """-> dict: q (Ns,P,D) and ref (No,Nt,P,D) unit rows with about 30 % masked (all-zero) patches; obj / best (Ns,) i64; qi (Ns,) i64,
    the query row each proposal reads: a permutation in which proposals 1 and 3 repeat the rows of proposals 0 and 2; ng / zq / zt as
    patch_roles names them.  The first half of each query row resembles randomly chosen patches of the template of the first proposal
    that reads it, with similarities spread over 0.2 .. 0.95: column maxima fall on both sides of every threshold.  Patches that miss
    a margin are masked until none does."""
    g = gen(3000 + seed + P + D + Ns)
    ref = _unit(torch.randn(No, Nt, P, D, generator=g))
    ref *= (torch.rand(No, Nt, P, 1, generator=g) > 0.3)
    q = _unit(torch.randn(Ns, P, D, generator=g))
    q *= (torch.rand(Ns, P, 1, generator=g) > 0.3)
    roles = patch_roles(Ns)
    ordinary = [p for p in range(Ns) if p not in roles.values()]
    # templates: the slices (0, 0) and (No-1, Nt-1) belong to zt and ng; proposal 0 reaches the last object at the last free template
    obj = torch.randint(0, No, (Ns,), generator=g)
    best = torch.randint(0, Nt, (Ns,), generator=g)
    for p in ordinary:
        if (int(obj[p]), int(best[p])) in ((0, 0), (No - 1, Nt - 1)):
            obj[p], best[p] = No - 1, 0
    obj[0], best[0] = No - 1, Nt - 2
    if roles["zt"] is not None:
        obj[roles["zt"]], best[roles["zt"]] = 0, 0
    if roles["ng"] is not None:
        obj[roles["ng"]], best[roles["ng"]] = No - 1, Nt - 1
    ref[0, 0] = 0
    ref[No - 1, Nt - 1] = _unit(torch.rand(P, D, generator=g) + 0.05)
    # query rows
    qi = torch.randperm(Ns, generator=g)
    for a, b in ((1, 0), (3, 2)):
        if a in ordinary and b in ordinary:
            qi[a] = qi[b]
    written = set()
    for p in ordinary:
        r = int(qi[p])
        if r in written:
            continue
        written.add(r)
        t = ref[int(obj[p]), int(best[p]), torch.randperm(P, generator=g)[: P // 2]]
        w = 0.2 + 0.75 * torch.rand(P // 2, 1, generator=g)
        mix = _unit(w * t + (1 - w * w).sqrt() * _unit(torch.randn(P // 2, D, generator=g)))
        q[r, : P // 2] = mix * (t != 0).any(-1, keepdim=True)
    if roles["zq"] is not None:
        q[int(qi[roles["zq"]])] = 0
    if roles["ng"] is not None:
        q[int(qi[roles["ng"]])] = -ref[No - 1, Nt - 1]
    for _ in range(20):  # mask what misses a margin
        red = patch_reduce64(q, ref, obj, best, qi)
        cm = red["colmax"]
        bad = (cm != 0) & (cm.abs() < 2 * MARGIN)
        for t in PATCH_THREDS:
            bad |= (cm - t).abs() < 2 * MARGIN
        badq = red["live"] & (red["rowsum"].abs() < 2 * MARGIN)
        if not bad.any() and not badq.any():
            break
        for p in range(Ns):
            ref[int(obj[p]), int(best[p]), bad[p]] = 0
            q[int(qi[p]), badq[p]] = 0
    return dict(q=q, ref=ref, obj=obj, best=best, qi=qi, **roles)


@functools.lru_cache(maxsize=None)
def patch_case(shape):
    """patch_inputs of one PATCH_SHAPES entry with its float64 reductions, built once per process"""
    d = patch_inputs(*shape)
    d["red"] = patch_reduce64(d["q"], d["ref"], d["obj"], d["best"], d["qi"])
    return d


def sim_inputs(P, D=36, Ns=4, seed=0):
    """sam6d_ism_patch_scores alone: q (Ns,P,D) unit rows with masked patches, sim (Ns,P,P) = the float64 product with as many other
    unit rows, rounded ONCE to fp32 -- the kernel and the float64 reference then reduce the same numbers.  Entries within the margin of
    a threshold or of zero are moved off it."""
    g = gen(3500 + seed + P)
    q = _unit(torch.randn(Ns, P, D, generator=g)) * (torch.rand(Ns, P, 1, generator=g) > 0.3)
    r = _unit(torch.randn(Ns, P, D, generator=g)) * (torch.rand(Ns, P, 1, generator=g) > 0.3)
    r[:, : P // 2] = _unit(0.9 * q[:, : P // 2] + 0.45 * _unit(torch.randn(Ns, P // 2, D, generator=g))) * (q[:, : P // 2] != 0).any(-1, keepdim=True)
    sim = (q.double() @ r.double().transpose(1, 2)).float()
    for t in PATCH_THREDS:
        near = (sim.double() - t).abs() < 2 * MARGIN
        sim[near] = float(t) + 4 * MARGIN
    sim[(sim != 0) & (sim.abs() < 2 * MARGIN)] = 0
    return q, sim


# ------------------------------------------------------------------------------------------------------------- projection
PROJ_IMAGES = [(50, 80), (48, 64), (100, 112), (480, 640), (50, 70)]  # the last one has W % 16 != 0: the general path
PROJ_NPC = (1, 255, 256, 257, 2048)
PROJ_NS = (1, 7, 8, 9, 17)
PROJ_SCALES = (0.1, 1.0, 10.0)
PROJ_MASKS = ("u8_1", "u8_255", "bool", "f32")


def proj_cases():
    """(H, W, Npc, Ns, mask kind, with mask_index, depth_scale): every image with every Npc; Ns, the mask kind and the depth scale cycle
    so that each value meets each image; mask_index alternates"""
    out = []
    for a, (H, W) in enumerate(PROJ_IMAGES):
        for j, npc in enumerate(PROJ_NPC):
            out.append((H, W, npc, PROJ_NS[(j + a) % 5], PROJ_MASKS[(j + a) % 4], bool((j + a // 2) % 2), PROJ_SCALES[(j + 2 * a) % 3]))
    return out


def random_rotation(g):
    qr = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64)).Q
    if torch.linalg.det(qr) < 0:
        qr[:, 0] = -qr[:, 0]
    return qr.float()


def camera(H, W):
    """K (3,3) float64 as the reference's caller passes it: the demo camera scaled to the image"""
    K = torch.tensor(CAM_K, dtype=torch.float64).reshape(3, 3).clone()
    K[0] *= W / 640.0
    K[1] *= H / 480.0
    return K


def translation64(masks, depth, K, depth_scale):
    """mean back-projected masked depth of every mask (Ns,H,W) bool over one depth map, rounded once to fp32"""
    return translate_maps64(masks.double() * depth.double()[None], K, depth_scale)


def projection64(best, obj, poses, pc, translate, K):
    """K32 (R p + t) / z in float64 from the fp32 inputs (the reference casts K to fp32 for this step) -> (Ns,Npc,2) f64, x then y"""
    R = poses[best, 0:3, 0:3].double()
    posed = torch.einsum("nij,nkj->nki", R, pc[obj].double()) + translate.double()[:, None, :]
    homo = torch.einsum("ij,nkj->nki", K.float().double(), posed)
    return homo[..., 0:2] / homo[..., 2:3]


def pixels(proj, H, W):
    """truncate toward zero and clamp to the image; -> (vu i32, keep bool): keep marks the coordinates at least PX_MARGIN from an integer"""
    vu = proj.trunc().clamp(min=-2.0 ** 31, max=2.0 ** 31 - 1).to(torch.int64)
    vu[..., 0].clamp_(0, W - 1)
    vu[..., 1].clamp_(0, H - 1)
    keep = (proj - proj.round()).abs() >= PX_MARGIN
    return vu.to(torch.int32), keep


def proj_inputs(H, W, Npc, Ns, kind, with_index, depth_scale, seed=0):
    """No = 3 clouds, 6 poses, rectangle masks over a depth map with zeros.  Mask 0 holds the image's first pixels (so that a lane
    beyond the image that wrongly read pixel 0 would count), proposal 1 (Ns >= 7) has an empty mask.  best / obj reach (5, 2) at
    proposal 0.  Cloud points whose float64 projection comes within PX_MARGIN of an integer for any proposal are drawn again."""
    g = gen(4000 + seed + H + 3 * W + Npc + 7 * Ns)
    No, Nt = 3, 6
    K = camera(H, W)
    depth = (700 + 300 * torch.rand(H, W, generator=g)).to(torch.int32)
    depth[torch.rand(H, W, generator=g) < 0.1] = 0
    depth[0, :16] = 800
    Nm = Ns + 2 if with_index else Ns
    masks = torch.zeros(Nm, H, W, dtype=torch.bool)
    for i in range(Nm):
        h, w = int(torch.randint(H // 4, H // 2, (1,), generator=g)), int(torch.randint(W // 4, W // 2, (1,), generator=g))
        y0, x0 = int(torch.randint(0, H - h, (1,), generator=g)), int(torch.randint(0, W - w, (1,), generator=g))
        masks[i, y0:y0 + h, x0:x0 + w] = True
    mi = None
    if with_index:
        mi = torch.randint(0, Nm, (Ns,), generator=g)
        mi[0] = 0
        if Ns > 2:
            mi[2] = mi[Ns - 1]
    first = 0
    masks[first, : H // 3, : W // 2] = True
    empty = 1 if Ns >= 7 else None
    if empty is not None:
        masks[1] = False
        if with_index:
            mi[mi == 1] = 0
            mi[empty] = 1
    best = torch.randint(0, Nt, (Ns,), generator=g)
    obj = torch.randint(0, No, (Ns,), generator=g)
    best[0], obj[0] = Nt - 1, No - 1
    poses = torch.eye(4).repeat(Nt, 1, 1)
    for i in range(Nt):
        poses[i, :3, :3] = random_rotation(g)
    poses[:, :3, 3] = torch.randn(Nt, 3, generator=g) * 0.4
    pc = (torch.rand(No, Npc, 3, generator=g) - 0.5) * 0.2 * float(depth_scale)
    sel_masks = masks[mi] if with_index else masks
    tr = translation64(sel_masks, depth, K, depth_scale)
    live = torch.ones(Ns, dtype=torch.bool)
    if empty is not None:
        live[empty] = False
    for _ in range(50):
        keep = pixels(projection64(best, obj, poses, pc, tr, K), H, W)[1]
        bad = torch.zeros(No, Npc, dtype=torch.bool)
        for p in range(Ns):
            if live[p]:
                bad[int(obj[p])] |= ~keep[p].all(-1)
        if not bad.any():
            break
        fresh = (torch.rand(No, Npc, 3, generator=g) - 0.5) * 0.2 * float(depth_scale)
        pc[bad] = fresh[bad]
    if kind == "u8_1":
        m = masks.to(torch.uint8)
    elif kind == "u8_255":
        m = masks.to(torch.uint8) * 255
    elif kind == "bool":
        m = masks.clone()
    else:
        m = masks.float()
    return dict(masks=m, sel_masks=sel_masks, mi=mi, depth=depth, K=K, depth_scale=float(depth_scale), poses=poses, pc=pc, best=best, obj=obj,
                translate=tr, live=live, H=H, W=W)


def projection_expect(d):
    """-> vu (Ns,Npc,2) i32, keep (Ns,Npc,2) bool, xyxy (Ns,4) i32, share of coordinates of live proposals left out"""
    vu, keep = pixels(projection64(d["best"], d["obj"], d["poses"], d["pc"], d["translate"], d["K"]), d["H"], d["W"])
    xyxy = torch.cat((vu.min(1).values, vu.max(1).values), -1)
    live = d["live"]
    share = float((~keep[live]).sum()) / max(int(keep[live].numel()), 1)
    return vu, keep, xyxy, share


def ulp_distance(a, b):
    """distance in units of the last place between two fp32 tensors of one sign pattern (0 where bit-equal)"""
    ia = a.contiguous().view(torch.int32).to(torch.int64)
    ib = b.contiguous().view(torch.int32).to(torch.int64)
    ia = torch.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = torch.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return (ia - ib).abs()


# ------------------------------------------------------------------------------------------------------------- translate_maps
MAP_SHAPES = [(1, 1), (7, 300), (33, 1), (257, 513)]


def map_inputs(N, H, W, seed=0):
    """N already-masked depth maps (mm, fp32) with zeros and negative values"""
    g = gen(5000 + seed + N + H + 3 * W)
    md = (700 + 300 * torch.rand(N, H, W, generator=g)).floor()
    r = torch.rand(N, H, W, generator=g)
    md[r < 0.3] = 0
    md[(r >= 0.3) & (r < 0.4)] *= -1
    if H * W == 1:
        md[0] = 812.0
    return md


def translate_maps64(md, K, depth_scale):
    """N masked depth maps (mm) -> (N,3) fp32: the mean of the back-projected pixels with Z > 0, every term and sum in float64, rounded
    once.  The denominator is the reference's `count_nonzero(valid) + 1e-8` as torch evaluates it: an int64 count plus a Python
    float is a float32 sum, so the 1e-8 survives only for an empty map."""
    N, H, W = md.shape
    u = torch.arange(W, dtype=torch.float64)[None, None, :]
    v = torch.arange(H, dtype=torch.float64)[None, :, None]
    Z = md.double() * float(depth_scale) / 1000
    valid = Z > 0
    Z = Z * valid
    n = (valid.sum((1, 2)).float() + 1e-8).double()
    X = ((u - K[0, 2]) * Z / K[0, 0]).sum((1, 2)) / n
    Y = ((v - K[1, 2]) * Z / K[1, 1]).sum((1, 2)) / n
    return torch.stack((X, Y, Z.sum((1, 2)) / n), 1).float()


# ------------------------------------------------------------------------------------------------------------- IoU / final score
IOU_NS = (0, 1, 255, 256, 257, 1000)


def iou_inputs(Ns, spoil=None, seed=0):
    """a (Ns,4) i32 projected boxes, b (Ns,4) i64 proposal boxes, all overlapping with a positive area: b contained in a, a partial
    overlap, and both with coordinates up to 2^20, in turn.  spoil = "touch": pair Ns // 2 shares an edge only (w = 0);
    spoil = "disjoint": that pair lies apart."""
    g = gen(6000 + seed + Ns)
    a = torch.zeros(Ns, 4, dtype=torch.int64)
    b = torch.zeros(Ns, 4, dtype=torch.int64)
    for i in range(Ns):
        big = (i % 3) == 2
        span = 2 ** 20 if big else 640
        x0, y0 = (int(v) for v in torch.randint(0, span // 2, (2,), generator=g))
        w, h = (int(v) for v in torch.randint(8, span // 2, (2,), generator=g))
        a[i] = torch.tensor([x0, y0, x0 + w, y0 + h])
        if i % 3 == 0:  # contained
            b[i] = torch.tensor([x0 + w // 4, y0 + h // 4, x0 + w // 4 + max(w // 2, 1), y0 + h // 4 + max(h // 2, 1)])
        else:           # partial overlap
            b[i] = torch.tensor([x0 + w // 2, y0 + h // 2, x0 + w + 5, y0 + h + 7])
    if spoil and Ns:
        i = Ns // 2
        x1 = int(a[i, 2])
        b[i] = torch.tensor([x1 if spoil == "touch" else x1 + 3, int(a[i, 1]), x1 + 10, int(a[i, 3])])
    return a.to(torch.int32), b


def iou64(a, b):
    """-> iou (Ns,) f64 (meaningful where positive), positive (Ns,) bool: the pairs whose overlap has a positive width and height"""
    a, b = a.to(torch.int64), b.to(torch.int64)
    wh = torch.min(a[:, 2:4], b[:, 2:4]) - torch.max(a[:, 0:2], b[:, 0:2])
    inter = (wh[:, 0] * wh[:, 1]).double()
    area = lambda x: ((x[:, 2] - x[:, 0]) * (x[:, 3] - x[:, 1])).double()
    return inter / (area(a) + area(b) - inter), (wh > 0).all(-1)


def final64(sem, appe, geo, vis):
    return (sem.double() + appe.double() + (geo.double() if torch.is_tensor(geo) else geo) * vis.double()) / (2 + vis.double())


def final_inputs(Ns, seed=0):
    """sem over Ns + 3 queries with a selection (Ns,) i32 into it, appe / geo / vis (Ns,) in [0,1]"""
    g = gen(6500 + seed + Ns)
    sem_all = torch.rand(Ns + 3, generator=g)
    sel = torch.randint(0, Ns + 3, (Ns,), generator=g).to(torch.int32)
    if Ns:
        sel[0] = Ns + 2
    return sem_all, sel, torch.rand(Ns, generator=g), torch.rand(Ns, generator=g), torch.rand(Ns, generator=g)
