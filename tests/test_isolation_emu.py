"""Row-isolation checks (tests/isolation.py, tests/isolation_cases.py) of the kernel SOURCES on the wave64 emulator, and the
tests of the method itself (plain torch, no kernel).  The emulator runs the narrower list; tests/test_isolation_gpu.py runs
the full table on the device, where the hand-overs between workgroups really are concurrent."""
import pytest
import torch

import isolation as I
import isolation_cases as IC
from isolation import Op


# ----------------------------------------------------------------------------- the method
def _seq_sum(x, reverse_last_row=False):
    """Row sums of fp32 ``x`` [M, n], added left to right; ``reverse_last_row``: the last row right to left."""
    acc = torch.zeros(x.shape[0], dtype=x.dtype)
    accr = torch.zeros(x.shape[0], dtype=x.dtype)
    for j in range(x.shape[1]):
        acc = acc + x[:, j]
        accr = accr + x[:, x.shape[1] - 1 - j]
    if reverse_last_row:
        acc = acc.clone()
        acc[-1] = accr[-1]
    return acc


def _row_op(name, fn, M=20, n=48, **kw):
    make = lambda dev: dict(x=torch.randn(M, n, generator=torch.Generator().manual_seed(1)))
    return Op(name, make, lambda i: dict(y=fn(i["x"])), (M,), dict(x=0), dict(y=0), **kw)


def _cumsum(x):
    acc, cols = torch.zeros(x.shape[0]), []
    for j in range(x.shape[1]):
        acc = acc + x[:, j]
        cols.append(acc)
    return torch.stack(cols, 1)


def test_method_masked_neighbour_fails_poisoned_only():
    """y = x + 0 * (the row above): invisible on finite data (permutation, subset and a tolerance all pass it), but the
    neighbour's NaN or inf arrives: 0 * NaN = NaN."""
    op = _row_op("x + 0 * neighbour", lambda x: x + 0 * x.roll(1, 0))
    x = op.make("cpu")
    I.check_permutation(op, x)
    I.check_subset(op, x)
    with pytest.raises(AssertionError, match=r"poisoned-neighbours check \(nan\)"):
        I.check_poisoned(op, x)


def test_method_slot_dependent_summation_order_fails_permutation():
    """The last slot sums in another order (a tail tile with its own reduction tree): within every tolerance, each row's
    neighbours do not matter (the poisoned check passes), but a row moved into the last slot changes bits."""
    op = _row_op("row sum, last slot reversed", lambda x: _seq_sum(x, reverse_last_row=True))
    x = op.make("cpu")
    torch.testing.assert_close(op.run(x)["y"], x["x"].double().sum(1).float(), rtol=1e-5, atol=1e-5)
    I.check_poisoned(op, x)
    with pytest.raises(AssertionError, match="permutation check"):
        I.check_permutation(op, x)
    I.check_permutation(_row_op("row sum", _seq_sum), x)


def test_method_batch_wide_softmax_shift_fails_poisoned_and_subset():
    """softmax with the maximum of the WHOLE batch as its shift: mathematically the same, every row within rounding of the
    per-row form -- and every row NaN once one row holds a NaN, and other bits when launched without the row that held
    the maximum."""
    def softmax_batch_shift(x):
        e = torch.exp(x - x.max())
        return e / e.sum(1, keepdim=True)
    op = _row_op("softmax, batch-wide shift", softmax_batch_shift)
    x = op.make("cpu")
    torch.testing.assert_close(op.run(x)["y"], torch.softmax(x["x"], 1), rtol=1e-5, atol=1e-7)
    with pytest.raises(AssertionError, match="poisoned-neighbours check"):
        I.check_poisoned(op, x)
    with pytest.raises(AssertionError, match="subset check"):
        I.check_subset(op, x)


def test_method_clean_op_passes_all_checks_and_a_look_ahead_fails_the_time_check():
    """A per-row causal op (running sum, left to right) passes all four checks and the in-place subset; the same op reading
    one position ahead fails the time-axis check exactly at the last position before t0."""
    t = dict(time_axes=dict(x=1, y=1), t0s=(13, 32), checks=("permutation", "poisoned", "subset", "subset_in_place", "time"))
    op = _row_op("running sum", _cumsum, **t)
    assert I.check_all(op, "cpu") == list(t["checks"])
    ahead = _row_op("running sum + 0.001 * next", lambda x: _cumsum(x) + 0.001 * x.roll(-1, 1), **t)
    with pytest.raises(AssertionError, match=r"time-axis check \(t0 = 13\).*positions \[12\]"):
        I.check_time(ahead, ahead.make("cpu"))


def test_method_unit_axes_and_choices():
    """The plumbing: (b, h) grids on two axes and merged into one, the fixed permutation (no fixed point, crosses 16-row
    tiles and the 64-row main / tail split), the victims (a survivor next to a victim), integer inputs, index ranges."""
    for n in (2, 3, 5, 6, 9, 17, 20, 40, 130):
        p = I.permutation(n)
        assert sorted(p.tolist()) == list(range(n)) and bool((p != torch.arange(n)).all())
        if n > 16:
            assert bool(((p // 16) != (torch.arange(n) // 16)).any())
        if n > 64:
            assert bool(((p >= 64) != (torch.arange(n) >= 64)).any())
        v = I.victims((n,))
        assert bool(v[0]) and not bool(v.all()) and bool((v[:-1] != v[1:]).any())
    B, H = 3, 2
    grid_op = Op("grid", lambda dev: dict(S=torch.randn(B, H, 4), hist=torch.randn(2, B * H, 4), idx=torch.arange(B * H).view(B, H)),
                 lambda i: dict(o=i["S"] * 2 + i["hist"].view(2, *i["S"].shape[:2], 4).sum(0), part=i["hist"] + 1, tok=i["idx"] % 3),
                 (B, H), dict(S=0, hist=I.Flat(1), idx=0), dict(o=0, part=I.Flat(1), tok=0),
                 alt_ints=lambda i: dict(idx=i["idx"] + 1), index_outputs=dict(tok=(0, 3)))
    I.check_all(grid_op, "cpu")
    leaky = Op("grid, heads mixed", grid_op.make, lambda i: dict(o=i["S"] + 0 * i["S"].flip(1), part=i["hist"], tok=i["idx"] % 3),
               (B, H), grid_op.inputs, grid_op.outputs, alt_ints=grid_op.alt_ints)
    with pytest.raises(AssertionError, match="poisoned-neighbours"):
        I.check_all(leaky, "cpu")
    out_of_range = Op("bad index", grid_op.make, grid_op.run, (B, H), grid_op.inputs, grid_op.outputs, alt_ints=grid_op.alt_ints,
                      index_outputs=dict(tok=(0, 2)))
    with pytest.raises(AssertionError, match="leaves"):
        I.check_all(out_of_range, "cpu")
    a, b = torch.tensor([0.0, float("nan")]), torch.tensor([-0.0, float("nan")])
    assert torch.equal(I.bits(a)[1:], I.bits(b)[1:]) and not torch.equal(I.bits(a)[:1], I.bits(b)[:1])


# ----------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("op", IC.table(gpu=False))
def test_isolation(emu, op):
    I.check_all(op, "cpu", repeat=False)


@pytest.mark.parametrize("B,d,dtype", IC.REARM)
def test_isolation_rows_rearm(emu, B, d, dtype):
    IC.check_rows_rearm("cpu", B, d, dtype)
