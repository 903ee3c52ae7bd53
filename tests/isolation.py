"""Row-isolation checks: the bits of a unit's outputs depend on nothing but that unit's inputs.

A *unit* is what ``generate_batch`` / ``generate_queue`` promise to keep apart: a batch row of the row-wise kernels, a (b, h)
pair of the state kernels.  An op under test is an ``Op``:

  * ``make(dev)`` builds the inputs once ({name: tensor}); ``run(inputs)`` launches the kernels through
    ``lina_speech_amd.ops`` and returns {name: tensor}.  ``run`` receives clones, reads its sizes from the shapes it is
    given (the checks hand it smaller batches), lays the tensors out as the launcher wants them and runs ALL steps of a
    multi-step op (a K1w window with its flush, two steps of the conv caches, the loop-control block over several steps).
    Fragment-major operands are built inside ``run`` with ``ops.pack_rows`` from the row-major tensor it is given and
    returned through ``ops.unpack_rows``, so the harness only ever sees row-major tensors;
  * ``units``: the unit grid, ``(B,)`` or ``(B, H)``;
  * ``inputs`` / ``outputs``: for every tensor the axis that indexes the unit -- an int (a 1-D grid: the row axis; a 2-D
    grid: the FIRST of two adjacent axes b, h), ``Flat(a)`` (a 2-D grid merged into one axis, as the K1w history
    ``[W, B*H, D]``) or ``None`` for what all units legitimately share (weights, positional tables, step counters; a shared
    OUTPUT, such as the stopped-rows count of the loop-control header, is excluded from every comparison and the case says
    why).  State ``[B, H, Dk, Dv]`` -> 0;  ``o_part [Dk/64, B, H, Dv]`` -> 1;  ``tok_log [steps, Q, B]`` -> 2.

Every comparison is on the BIT PATTERNS (an integer view): NaN == NaN, -0 != +0, no tolerance.  The four checks:

  1. ``check_permutation``: every unit-indexed input permuted by one fixed permutation (no fixed point; it moves units
     across the 16-row tiles and across the main / tail split of the row count) -- the outputs, permuted back, are those of
     the first run.
  2. ``check_poisoned``: the victims (every second unit, the first and the last; at least one survivor sits next to a victim
     in the same 16-row tile / head pair) get NaN -- in a second variant +inf and 3e38, mixed -- in every floating
     unit-indexed input and state, and OTHER VALID values in their integer inputs (``alt_ints``); every output slice of
     every survivor is unchanged.  Outputs of victims are not compared; where they are indices (``index_outputs``) they must
     stay in range, for every unit.
  3. ``check_subset``: the survivors launched as a smaller batch, and one unit launched alone, with the same kernel
     variant (``run`` keeps ``force`` / ``variant`` / ``n_wg`` / ``nseg``) -- equal to the same units' slices of the full launch.
     ``check_subset_in_place`` is its form for ops that legitimately take the unit's INDEX and the unit count into the result
     (the hashed uniforms of the sampling kernels): same slots, same launch size, every other slot overwritten.
  4. ``check_time`` (causal sequence ops only: ``time_axes``): the inputs at positions >= t0 replaced by OTHER FINITE values
     (the originals times 0.5); the outputs at positions < t0 are unchanged.  Outputs without a time axis (a final state)
     are not compared.  FINITE ONLY, on purpose: a chunked kernel forms the masked product tril(q k^T) v of a whole
     32-token chunk in MFMA, and 0 x NaN of a masked-out future position is NaN -- the full-head bf16 K2 at T = 100 puts
     NaN into positions 32..44 when positions >= 45 are NaN (clean at t0 = 64, a chunk edge).  For finite data that product
     is exact zero, and finite data is all a causal sequence kernel promises.

A failing check raises AssertionError naming the op, the check, the tensor and the first differing units.
"""
import dataclasses
from typing import Callable, Optional

import torch


@dataclasses.dataclass(frozen=True)
class Flat:
    """A 2-D unit grid merged into ONE axis (index b * H + h)."""
    axis: int


@dataclasses.dataclass
class Op:
    name: str
    make: Callable          # dev -> {name: tensor}
    run: Callable           # {name: tensor} -> {name: tensor}
    units: tuple            # (B,) or (B, H)
    inputs: dict            # name -> unit axis | Flat | None
    outputs: dict           # name -> unit axis | Flat | None
    checks: tuple = ("permutation", "poisoned", "subset")
    alt_ints: Optional[Callable] = None     # inputs -> {name: tensor of other valid values} for integer unit inputs
    index_outputs: dict = dataclasses.field(default_factory=dict)     # name -> (lo, hi) inclusive / exclusive
    time_axes: dict = dataclasses.field(default_factory=dict)         # input and output name -> time axis
    t0s: tuple = ()
    # the subset check hands ``run`` the chosen units as a batch of this shape: ``None`` -> (n,) for rows, and for a
    # (B, H) grid whole batch rows [B', H] plus one (b, h) as [1, 1]; "rows" -> whole batch rows only (kernels whose form is
    # chosen by H: the single unit is then one b with all its heads)
    subset_units: Optional[str] = None
    note: str = ""


# ----------------------------------------------------------------------------- unit-axis plumbing
def _n_units(grid):
    n = 1
    for g in grid:
        n *= g
    return n


def _flatten(t, spec, grid):
    """(view of ``t`` with the unit grid merged into one axis, that axis)."""
    if isinstance(spec, Flat):
        assert t.shape[spec.axis] == _n_units(grid), f"axis {spec.axis} of {tuple(t.shape)} is not the {grid} grid"
        return t, spec.axis
    a = spec
    assert tuple(t.shape[a:a + len(grid)]) == tuple(grid), f"axes {a}.. of {tuple(t.shape)} are not the {grid} grid"
    if len(grid) == 1:
        return t, a
    return t.reshape(*t.shape[:a], _n_units(grid), *t.shape[a + len(grid):]), a


def _unflatten(t, spec, grid, a):
    if isinstance(spec, Flat) or len(grid) == 1:
        return t
    return t.reshape(*t.shape[:a], *grid, *t.shape[a + 1:])


def take_units(tensors, specs, grid, idx, new_grid):
    """Every unit-indexed tensor of ``tensors`` reduced to / reordered as the flat units ``idx``, seen as ``new_grid``."""
    out = {}
    for name, t in tensors.items():
        spec = specs[name]
        if spec is None or t is None:
            out[name] = t
            continue
        f, a = _flatten(t, spec, grid)
        out[name] = _unflatten(f.index_select(a, idx.to(f.device)), spec, new_grid, a)
    return out


def bits(t):
    """The bit pattern of a tensor as integers (floating types through a view: NaN == NaN, -0 != +0)."""
    t = t.detach().cpu().contiguous()
    if t.is_floating_point():
        return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def _clone(tensors):
    return {k: (None if v is None else v.clone()) for k, v in tensors.items()}


def _run(op, tensors):
    out = op.run(_clone(tensors))
    missing = set(op.outputs) ^ set(out)
    assert not missing, f"{op.name}: outputs {sorted(missing)} are not declared / not returned"
    return out


def _compare(op, check, got, want, specs, grid, units=None, what=""):
    """``got`` == ``want`` bit for bit on every unit-indexed tensor; ``units``: flat units to look at (default all)."""
    for name, spec in specs.items():
        if spec is None or want[name] is None:
            continue
        g, a = _flatten(got[name], spec, grid)
        w, _ = _flatten(want[name], spec, grid)
        assert g.shape == w.shape and g.dtype == w.dtype, f"{op.name} {check}: {name} {tuple(g.shape)} {g.dtype} vs " \
                                                          f"{tuple(w.shape)} {w.dtype}"
        if units is not None:
            g, w = g.index_select(a, units.to(g.device)), w.index_select(a, units.to(w.device))
        diff = bits(g) != bits(w)
        if bool(diff.any()):
            bad = diff.movedim(a, 0).reshape(diff.shape[a], -1).any(1).nonzero().view(-1)
            if units is not None:
                bad = units[bad]
            first = tuple(diff.nonzero()[0].tolist())
            raise AssertionError(f"{op.name}: {check} check{what}: output {name!r} differs in {int(diff.sum())} elements, units "
                                 f"{bad.tolist()[:8]} of grid {tuple(grid)}; first at {first}: got {g[first].item()!r}, "
                                 f"want {w[first].item()!r}")


def _check_indices(op, out, what):
    for name, (lo, hi) in op.index_outputs.items():
        t = out[name]
        assert bool(((t >= lo) & (t < hi)).all()), f"{op.name}: {what}: {name} leaves [{lo}, {hi})"


# ----------------------------------------------------------------------------- the fixed choices
def permutation(n):
    """One fixed permutation of n >= 2 units without a fixed point that crosses every aligned block boundary: unit i goes to
    (i * s + c) mod n with s coprime to n (neighbours are pulled apart, so tiles and the main / tail split are crossed)."""
    import math
    assert n >= 2
    i = torch.arange(n)
    for s in (7, 5, 3, 11, 13, 9):
        if s < n and math.gcd(s, n) == 1:
            for c in (n // 2 + 1, 1, 2, 3):
                perm = (i * s + c) % n
                if bool((perm != i).all()):
                    return perm
    return (i + 1) % n                  # tiny grids: a rotation


def victims(grid):
    """Boolean mask over the flat units: every second unit, the first and the last.  With >= 3 units unit 1 survives next to
    the victims 0 and 2 (same 16-row tile, or the other head of a pair); with 2 units only the first is a victim."""
    n = _n_units(grid)
    assert n >= 2
    v = torch.zeros(n, dtype=torch.bool)
    v[::2] = True
    if n > 2:
        v[-1] = True
    if n == 3:
        v[2] = False           # 0 victim, 1 and 2 survive
    assert bool(v.any()) and bool((~v).any())
    return v


def _poison_value(t, variant):
    if variant == "nan":
        return torch.full_like(t, float("nan"))
    i = torch.arange(t.numel(), device=t.device).view(t.shape)
    mixed = torch.where(i % 2 == 0, torch.full_like(t, float("inf")), torch.full_like(t, 3e38))
    return torch.where(i % 3 == 0, -mixed, mixed)


def _unit_mask(t, spec, grid, mask):
    f, a = _flatten(t, spec, grid)
    shape = [1] * f.dim()
    shape[a] = mask.numel()
    return _unflatten(mask.to(t.device).view(shape).expand(f.shape), spec, grid, a).reshape(t.shape)


# ----------------------------------------------------------------------------- the four checks
def check_permutation(op, inputs, base=None):
    grid = op.units
    base = _run(op, inputs) if base is None else base
    perm = permutation(_n_units(grid))
    got = _run(op, take_units(inputs, op.inputs, grid, perm, grid))
    _check_indices(op, got, "permuted run")
    _compare(op, "permutation", got, take_units(base, op.outputs, grid, perm, grid), op.outputs, grid)
    return base


def check_poisoned(op, inputs, base=None):
    grid = op.units
    base = _run(op, inputs) if base is None else base
    vic = victims(grid)
    survivors = (~vic).nonzero().view(-1)
    alt = op.alt_ints(inputs) if op.alt_ints else {}
    n_float = 0
    for variant in ("nan", "inf"):
        bad = {}
        for name, t in inputs.items():
            spec = op.inputs[name]
            if spec is None or t is None:
                bad[name] = t
            elif t.is_floating_point():
                bad[name] = torch.where(_unit_mask(t, spec, grid, vic), _poison_value(t, variant), t)
                n_float += 1
            else:
                assert name in alt, f"{op.name}: no other valid values given for the integer unit input {name!r}"
                assert alt[name].shape == t.shape and alt[name].dtype == t.dtype
                bad[name] = torch.where(_unit_mask(t, spec, grid, vic), alt[name], t)
        got = _run(op, bad)
        _check_indices(op, got, f"poisoned run ({variant})")
        _compare(op, "poisoned-neighbours", got, base, op.outputs, grid, units=survivors, what=f" ({variant})")
    assert n_float or alt, f"{op.name}: nothing to poison"
    return base


def _subsets(op):
    """[(flat units, grid of the smaller launch)]"""
    grid = op.units
    n = _n_units(grid)
    vic = victims(grid)
    if len(grid) == 1:
        return [((~vic).nonzero().view(-1), None), (torch.tensor([n // 2]), None)]
    B, H = grid
    allh = torch.arange(H)
    rows = torch.arange(B)[1::2] if B > 1 else torch.arange(1)          # every second batch row, with all its heads
    res = []
    if B > 1:
        res.append(((rows[:, None] * H + allh[None, :]).reshape(-1), (len(rows), H)))
    b1 = B - 1
    if op.subset_units == "rows":
        if B > 1:
            res.append((b1 * H + allh, (1, H)))
    else:
        res.append((torch.tensor([b1 * H + H // 2]), (1, 1)))
    assert res, f"{op.name}: no smaller launch exists for the grid {grid}"
    return res


def check_subset(op, inputs, base=None):
    grid = op.units
    base = _run(op, inputs) if base is None else base
    for idx, new_grid in _subsets(op):
        new_grid = (len(idx),) if new_grid is None else new_grid
        got = _run(op, take_units(inputs, op.inputs, grid, idx, new_grid))
        _check_indices(op, got, f"launch of units {idx.tolist()}")
        want = take_units(base, op.outputs, grid, idx, new_grid)
        _compare(op, "subset", got, want, op.outputs, new_grid, what=f" (units {idx.tolist()[:6]}.. as grid {new_grid})")
    return base


def check_subset_in_place(op, inputs, base=None):
    """The subset check for ops whose result legitimately depends on the unit's INDEX and on the unit count (hashed uniforms
    of the sampling kernels): the chosen units stay in their slots of a launch of the same size, every other slot is
    overwritten with a copy of the first chosen unit's inputs."""
    grid = op.units
    n = _n_units(grid)
    base = _run(op, inputs) if base is None else base
    vic = victims(grid)
    for idx in ((~vic).nonzero().view(-1), torch.tensor([n // 2])):
        src = torch.full((n,), int(idx[0]))
        src[idx] = idx
        got = _run(op, take_units(inputs, op.inputs, grid, src, grid))
        _check_indices(op, got, f"launch with only units {idx.tolist()} kept")
        _compare(op, "subset (in place)", got, base, op.outputs, grid, units=idx, what=f" (units {idx.tolist()[:6]}.. kept)")
    return base


def check_time(op, inputs, base=None):
    assert op.time_axes and op.t0s, f"{op.name}: no time axis declared"
    base = _run(op, inputs) if base is None else base
    compared = 0
    for t0 in op.t0s:
        later = {}
        for name, t in inputs.items():
            ax = op.time_axes.get(name)
            if ax is None or t is None:
                later[name] = t
                continue
            assert t.is_floating_point() and 0 < t0 < t.shape[ax]
            shape = [1] * t.dim()
            shape[ax] = t.shape[ax]
            after = (torch.arange(t.shape[ax], device=t.device) >= t0).view(shape)
            later[name] = torch.where(after, t * 0.5, t)
        got = _run(op, later)
        for name in op.outputs:
            ax = op.time_axes.get(name)
            if ax is None or base[name] is None:
                continue                      # no time axis (a final state): depends on all positions
            g, w = got[name].narrow(ax, 0, t0), base[name].narrow(ax, 0, t0)
            diff = bits(g) != bits(w)
            compared += 1
            if bool(diff.any()):
                pos = diff.movedim(ax, 0).reshape(t0, -1).any(1).nonzero().view(-1)
                raise AssertionError(f"{op.name}: time-axis check (t0 = {t0}): output {name!r} differs at positions "
                                     f"{pos.tolist()[:8]} < t0 after the inputs at >= t0 changed")
    assert compared, f"{op.name}: no output carries a time axis"
    return base


CHECKS = {"permutation": check_permutation, "poisoned": check_poisoned, "subset": check_subset, "time": check_time,
          "subset_in_place": check_subset_in_place}


def check_all(op, dev, only=None, repeat=True):
    """Every check the op lists (``only``: restrict to these), on one shared, unchanged base run.  ``repeat``: run the op twice
    first and compare (on the device a race shows as a run that differs from itself; the emulator is sequential)."""
    inputs = op.make(dev)
    missing = set(op.inputs) ^ set(inputs)
    assert not missing, f"{op.name}: inputs {sorted(missing)} are not declared / not made"
    base = _run(op, inputs)
    if repeat:
        _compare(op, "repeat", _run(op, inputs), base, op.outputs, op.units)
    _check_indices(op, base, "base run")
    keep = _clone(base)
    ran = []
    for name in op.checks:
        if only is None or name in only:
            CHECKS[name](op, inputs, base)
            ran.append(name)
    _compare(op, "base-unchanged", base, keep, op.outputs, op.units)
    return ran
