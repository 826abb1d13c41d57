"""The device draw of sam6d_hip.inputs (draw_choice, DeviceChoice) without a GPU: the numpy restatement tests/choice_ref.py against the
anchors of its definition, the bijection that rules out ties, the uniformity of the definition itself, and what the package refuses
before any launch."""
import numpy as np
import pytest
import torch

from tests import choice_ref as R


def test_anchors():
    assert ["%08x" % v for v in R.keys(1, 0, np.arange(4))] == ["d3c728c6", "95afc7b6", "40ba9132", "49a858b6"]
    assert R.draw_row(1, 2, 10, 3).tolist() == [8, 5, 4]
    assert R.draw_row(0, 0, 5, 8).tolist() == [2, 4, 2, 0, 3, 2, 3, 1]
    assert R.draw_row(12345, 6, 230400, 4).tolist() == [129555, 25593, 13006, 159492]
    assert R.draw_row(3, 1, 1166400, 5000)[:3].tolist() == [703137, 463947, 127901]


def test_edge_rows_and_batched_forms_agree():
    assert R.draw_row(5, 0, 0, 7).tolist() == [0] * 7 and R.draw_row(5, 0, -3, 7).tolist() == [0] * 7
    assert R.draw_row(5, 9, 1, 7).tolist() == [0] * 7
    assert R.draw_row(5, 9, 7, 7).max() < 7  # n == ns: with replacement, as the reference's `n <= ns`
    got = R.draw([0, 1, 6, 7, 8, 14, 300], 7, 11, row0=3)
    assert got.shape == (7, 7) and got.dtype == np.int32
    for i, n in enumerate([0, 1, 6, 7, 8, 14, 300]):
        assert np.array_equal(got[i], R.draw_row(11, 3 + i, n, 7))
        if n > 7:
            assert len(set(got[i].tolist())) == 7 and got[i].max() < n
    assert np.array_equal(R.draw_rows(11, np.arange(3, 6), 300, 7), R.draw([300] * 3, 7, 11, row0=3))
    assert np.array_equal(R.draw_rows(11, np.arange(3, 6), 5, 7), R.draw([5] * 3, 7, 11, row0=3))


@pytest.mark.parametrize("seed, row", [(0, 0), (1, 7), (12345, 0xFFFFFFFF)])
def test_keys_are_a_bijection(seed, row):
    h = R.keys(seed, row, np.arange(230400))
    assert h.max() < 1 << 32 and np.unique(h).size == 230400


def _p_value(stat, dof):
    """upper tail of the chi-square distribution: Q(dof / 2, stat / 2)"""
    return float(torch.special.gammaincc(torch.tensor(dof / 2.0, dtype=torch.float64), torch.tensor(stat / 2.0, dtype=torch.float64)))


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_definition_is_uniform(seed):
    """Chi-square p >= 0.01 for: the inclusion counts of the 1000 candidates over rows 0 .. 19999 at ns = 100 (without replacement the
    count of a candidate has variance R p (1 - p), p = ns / n: the hypergeometric factor 1 - ns / n), the distribution of sel[0] over
    the same rows (FPS starts from it), and the bin counts of the draw with replacement at n = 37, ns = 2048 over 200 rows."""
    n, ns, rows = 1000, 100, 20000
    inc, first = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for r0 in range(0, rows, 2000):
        s = R.draw_rows(seed, np.arange(r0, r0 + 2000), n, ns)
        inc += np.bincount(s.ravel(), minlength=n)
        first += np.bincount(s[:, 0], minlength=n)
    e = rows * ns / n
    p_inc = _p_value(((inc - e) ** 2).sum() / (e * (1 - ns / n)), n - 1)
    e = rows / n
    p_first = _p_value(((first - e) ** 2).sum() / e, n - 1)
    c = np.bincount(R.draw_rows(seed, np.arange(200), 37, 2048).ravel(), minlength=37)
    e = 200 * 2048 / 37
    p_repl = _p_value(((c - e) ** 2).sum() / e, 36)
    print("seed %d: p inclusion %.3f, first %.3f, with replacement %.3f" % (seed, p_inc, p_first, p_repl))
    assert min(p_inc, p_first, p_repl) >= 0.01, (p_inc, p_first, p_repl)


def test_refusals():
    from sam6d_hip import _lib, inputs
    n = torch.tensor([10, 20], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device"):
        inputs.draw_choice(n, 4, 0)
    for ns in (0, 8193, -1):
        with pytest.raises(ValueError, match="8192"):
            inputs.draw_choice(n, ns, 0)
        with pytest.raises(RuntimeError, match="draw_choice"):  # the C entry refuses the size itself, before it looks at a pointer
            _lib.call("sam6d_draw_choice", None, 0, ns, 0, 0, None, None)
    with pytest.raises(RuntimeError, match="draw_choice"):
        _lib.call("sam6d_draw_choice", None, -1, 4, 0, 0, None, None)
    _lib.call("sam6d_draw_choice", None, 0, 4, 0, 0, None, None)  # N == 0 with null pointers: a no-op


def test_device_choice_row_advances_by_the_rows_drawn(monkeypatch):
    from sam6d_hip import inputs
    calls = []

    def fake(n, ns, seed, row0=0):
        calls.append((int(n.shape[0]), ns, seed, row0))
        return torch.zeros((n.shape[0], ns), dtype=torch.int32)

    monkeypatch.setattr(inputs, "draw_choice", fake)
    rng = inputs.DeviceChoice(7)
    assert (rng.seed, rng.row) == (7, 0)
    rng.draw(torch.zeros(12, dtype=torch.int32), 64)
    assert rng.row == 12
    rng.draw(torch.zeros(3, dtype=torch.int32), 5000)
    assert rng.row == 15
    rng.draw(torch.zeros(0, dtype=torch.int32), 8)
    assert rng.row == 15
    assert calls == [(12, 64, 7, 0), (3, 5000, 7, 12), (0, 8, 7, 15)]
