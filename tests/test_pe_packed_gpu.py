"""The counted PositionalEncoding entry (sam6d_pe_mlp_max_counted: real ball neighbours packed into MFMA tiles, padded slots skipped)
against the existing entry on the same indices -- bit for bit -- and the ball query that reports the counts.

The contract of the counted entry (include/sam6d_hip.h): 1 <= cnt[p] <= S, and every slot l >= cnt[p] of a point repeats an index of a
slot < cnt[p].  Every idx below is built to satisfy it; the reference result comes from sam6d_pe_mlp_max, which ignores counts."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 32),       # less than one block of 8 points
          (3, 701, 32),     # N no multiple of the block: blocks straddle clouds
          (2, 1500, 64),
          (40, 2048, 32)]   # more than one pass of the persistent grid (10240 blocks over 3072 waves)
PATTERNS = ["hits", "empty", "full", "stride"]


@pytest.fixture(scope="module")
def W(dev):
    from sam6d_hip import pem, synth
    return pem.PemWeights(synth.make_pem_weights(1), dev)


def _layers(W, S):
    return W.pe["mlp"][0 if S == 32 else 1]


def _args(L):
    return [L[i][k].data_ptr() for i in range(3) for k in ("w", "scale", "shift")]


def _run(entry, pts_d, idx_d, B, N, S, L, tail):
    """out (B*N, 256) preset to -7, the 128 features written at column 128."""
    from sam6d_hip import _lib
    out = torch.full((B * N, 256), -7.0, device=pts_d.device)
    _lib.call(entry, pts_d.data_ptr(), idx_d.data_ptr(), B, N, S, *_args(L), out.data_ptr(), 256, 128, *tail,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu()


def _check_counted(pts, idx, cnt, L, dev, fp64):
    B, N, S = idx.shape
    pts_d, idx_d, cnt_d = pts.to(dev), idx.to(dev), cnt.to(dev)
    want = _run("sam6d_pe_mlp_max", pts_d, idx_d, B, N, S, L, [])
    got = _run("sam6d_pe_mlp_max_counted", pts_d, idx_d, B, N, S, L, [0, cnt_d.data_ptr()])
    assert float((got[:, :128] + 7.0).abs().max()) == 0.0, "columns outside [off, off+128) were touched"
    assert torch.isfinite(got[:, 128:]).all()
    assert torch.equal(got[:, 128:], want[:, 128:]), "counted kernel differs from sam6d_pe_mlp_max: %d of %d values, max %.3e" % (
        int((got[:, 128:] != want[:, 128:]).sum()), got[:, 128:].numel(), float((got[:, 128:] - want[:, 128:]).abs().max()))
    if fp64:
        nb = torch.gather(pts.double()[:, None].expand(B, N, N, 3), 2, idx.long()[..., None].expand(B, N, S, 3))
        h = torch.cat([nb - (pts.double()[:, :, None] + 1e-8), nb], -1)
        for l in L:
            h = (h @ l["w"].double().cpu().t() * l["scale"].double().cpu() + l["shift"].double().cpu()).clamp(min=0)
        ref = h.max(2).values.reshape(B * N, 128)
        d = float((got[:, 128:].double() - ref).abs().max())
        print("\ncounted pe_mlp_max vs float64, B %d N %d S %d: max abs diff %.2e" % (B, N, S, d))
        assert d <= 2e-5, "counted pe_mlp_max vs float64: max abs diff %.3e > 2e-5" % d


def _pattern(kind, B, N, S, gen):
    """(idx (B,N,S) i32, cnt (B,N) i32) that satisfy the contract."""
    slot = torch.arange(S)[None, None]
    if kind == "empty":  # every ball empty: all slots index 0, one row counted
        return torch.zeros(B, N, S, dtype=torch.int32), torch.ones(B, N, dtype=torch.int32)
    if kind == "full":   # nothing padded: arbitrary indices
        return torch.randint(0, N, (B, N, S), generator=gen, dtype=torch.int32), torch.full((B, N), S, dtype=torch.int32)
    if kind == "hits":   # what a ball query returns: strictly increasing hits, then copies of the first
        kmax = min(S, N)
        cnt = torch.randint(1, kmax + 1, (B, N), generator=gen)
        val = torch.randint(1, N // kmax + 1, (B, N, S), generator=gen).cumsum(-1) - 1  # strictly increasing, < N in the first kmax slots
    else:                # "stride": counts 1 + (7 p mod S) hit 7, 8, 9, 16, 17, ...; item totals that are no multiple of 4
        cnt = 1 + (7 * torch.arange(B * N).reshape(B, N)) % S
        val = torch.randint(0, N, (B, N, S), generator=gen)
    idx = torch.where(slot < cnt[..., None], val, val[..., :1])
    assert int(idx.min()) >= 0 and int(idx.max()) < N
    return idx.to(torch.int32), cnt.to(torch.int32)


@pytest.mark.parametrize("kind", PATTERNS)
@pytest.mark.parametrize("B,N,S", SHAPES)
def test_counted_kernel_equals_existing_entry(dev, W, B, N, S, kind):
    gen = torch.Generator().manual_seed(B * 1000 + N + S + 7 * PATTERNS.index(kind))
    pts = torch.rand(B, N, 3, generator=gen) - 0.5
    idx, cnt = _pattern(kind, B, N, S, gen)
    if kind == "stride":
        assert {7, 8, 9, 16, 17} <= set(cnt.flatten().tolist()) or B * N < 32
    _check_counted(pts, idx, cnt, _layers(W, S), dev, fp64=B * N * S <= 4_000_000)


def test_ball_query_counts_and_counted_kernel(dev, W):
    """sam6d_ball_query2_grid_counts: the indices of the plain entry, counts equal to the host recount, and -- fed to the counted
    kernel -- the features of the plain kernel.  The queries reach beyond the cloud, so that empty, partial and full balls all occur."""
    from sam6d_hip import _lib
    B, N, r1, ns1, r2, ns2 = 2, 600, 0.12, 32, 0.5, 64
    gen = torch.Generator().manual_seed(600)
    pts = torch.rand(B, N, 3, generator=gen)
    new = torch.rand(B, N, 3, generator=gen) * 2.4 - 0.7
    pts_d, new_d = pts.to(dev), new.to(dev)
    nbytes = int(_lib.load().sam6d_ball_query2_grid_workspace_bytes(B, N))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    old = [torch.full((B, N, ns), -1, dtype=torch.int32, device=dev) for ns in (ns1, ns2)]
    idx = [torch.full((B, N, ns), -1, dtype=torch.int32, device=dev) for ns in (ns1, ns2)]
    cnt = [torch.full((B, N), -1, dtype=torch.int32, device=dev) for _ in range(2)]
    _lib.call("sam6d_ball_query2_grid", new_d.data_ptr(), pts_d.data_ptr(), B, N, N, r1, ns1, old[0].data_ptr(), r2, ns2, old[1].data_ptr(),
              ws.data_ptr(), nbytes, st)
    _lib.call("sam6d_ball_query2_grid_counts", new_d.data_ptr(), pts_d.data_ptr(), B, N, N, r1, ns1, idx[0].data_ptr(), r2, ns2,
              idx[1].data_ptr(), ws.data_ptr(), nbytes, cnt[0].data_ptr(), cnt[1].data_ptr(), st)
    torch.cuda.synchronize()
    d2 = ((new.double()[:, :, None] - pts.double()[:, None]) ** 2).sum(-1)
    seen = set()
    for k, (r, ns) in enumerate(((r1, ns1), (r2, ns2))):
        i, c = idx[k].cpu(), cnt[k].cpu()
        assert torch.equal(i, old[k].cpu()), "indices differ from sam6d_ball_query2_grid"
        assert torch.equal(c, (1 + (i[..., 1:] != i[..., :1]).sum(-1)).to(torch.int32)), "counts differ from the host recount"
        surely_empty = (d2 > r * r * 1.01).all(-1)  # no point within the radius, with room for fp32 rounding
        assert bool((c[surely_empty] == 1).all()) and bool((i[surely_empty] == 0).all()), "an empty ball must count 1 over zeros"
        seen |= {"empty"} if bool(surely_empty.any()) else set()
        seen |= {"partial"} if bool(((c > 1) & (c < ns)).any()) else set()
        seen |= {"full"} if bool((c == ns).any()) else set()
        _check_counted(pts, i, c, _layers(W, ns), dev, fp64=False)
    assert seen == {"empty", "partial", "full"}, seen
