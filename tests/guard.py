"""Guard bands around test tensors: does a kernel stay inside its tensors?

The parity checks of this suite compare what a kernel writes INSIDE its outputs.  A store past the end of an output (a tail
tile, the last partial 16-byte vector of a row, a row beyond M) and a load past the end of an input that reaches the
arithmetic (a full-width vector load followed by ``x * mask``: ``0 * finite`` hides what ``0 * NaN`` shows) pass every one of
them.  ``GuardArena`` hands out tensors that sit between two bands of known bytes, and ``guarded`` routes the tensors of an
unchanged case function (tests/kernel_cases.py and friends) and the outputs the launchers allocate themselves into such an arena.

Layout of one guarded tensor (its own allocation)::

    [ front band >= BAND bytes | tensor (starts on a 256-byte boundary, as a torch allocation does) | back band >= BAND bytes ]

The back band starts at the very next byte after the last element: there is no round-up slack.  ``BAND`` is 64 KiB: eight
rows of the widest row of the kernel cases (4112 bf16 columns) -- a stray row, a stray 16-byte vector, a stray window-history
slot or a row tile beyond M of the small shapes land inside it.  DAMAGE FARTHER AWAY THAN ONE BAND IS NOT SEEN.

Band contents: a kernel that wrongly consumes a band must be shown up but not led to a far address --
floating (and complex) types: all-ones bytes = NaN; integer and bool types: the element value 1 (a valid token id, length and
step).  ``empty`` / ``empty_like`` tensors hold the same fill in their body (torch leaves it undefined), so an output element
that no kernel wrote is NaN as well.

``check()`` compares every band bit for bit with its fill (through an integer view: NaN != NaN) and names the tensor (shape,
dtype, creation site or label), the side, the byte offset of the first damaged byte relative to the tensor's first byte
(negative: in front of it; >= its size: behind it) and the number of damaged bytes.

What ``guarded`` routes into the arena while it is active (everything is restored by pytest's monkeypatch):
  * ``tensor.to(dev)`` in its single-argument device form (``dev`` a str or torch.device of the arena's device type) -- how the
    case functions put their inputs on ``dev`` (on the emulator ``.to("cpu")`` returns the tensor itself: it is COPIED into the
    arena);
  * ``tensor.clone()`` (no arguments) of a tensor that already lives in the arena -- the states, conv caches and residual
    streams the cases clone before a kernel updates them in place;
  * the factory functions ``empty / zeros / ones / full / tensor / arange / randn / rand / randint`` called with a ``device=`` of
    the arena's type and ``empty_like / zeros_like / ones_like / full_like`` of a tensor on it, called through the ``torch``
    global of the case modules and of the launcher modules (``lina_speech_amd.kernels``, ``autograd``, ``backend``, ``train``,
    ``policy``): a proxy object stands in for that global.  The package's cached scratch (``ops.clear_workspaces()``: the
    segment states of the segment-parallel K2 / K2b, the padded channel-mixer weights) is dropped on entry and on exit, so a
    case allocates it anew, inside the arena, and nothing of an arena stays cached;
  * the result of ``ops.pack_rows(t)`` (an explicit seam: the fragment-major operands are built by ``permute`` + ``reshape``, which
    nothing above sees, and they are what the packed and the tall projection kernels load -- the weight panels by DMA -- and,
    for a packed residual stream, what they update in place).

NOT guarded (these tensors come from the ordinary allocator):
  * results of tensor methods and operators: ``contiguous()`` where it copies, ``float()`` / ``to(dtype)``, ``t()`` + ``contiguous``,
    ``reshape`` where it copies, ``torch.cat`` / ``stack``, arithmetic (``w * gamma``, ``x + r``), ``sum``, ``new_empty`` ...: e.g. the
    folded weights ``c1`` / ``c2`` of the projection cases, ``unpack_rows`` results, ``gk.float()``;
  * clones of tensors that require grad, clones with arguments, ``detach()`` alone (a view of the same memory: as guarded as
    its source);
  * tensors that require grad when they are moved (``.to(dev)`` of a graph node), gradients that autograd accumulates itself
    (``leaf.grad`` is autograd's own copy unless the backward's output is taken over as it is);
  * anything allocated by modules other than those listed (``decode.py``, the model classes) and by torch itself (``F.linear``,
    ``torch.optim``); module parameters (``Module.to`` uses the three-argument form of ``Tensor.to``);
  * views share the bands of their base: a kernel that leaves a column slice but stays inside the base tensor is not seen here
    (the ``"att log: something else was written"`` checks of the cases cover that).
Operands at unusual base alignments are out of scope: every guarded tensor starts on a 256-byte boundary.
"""
import contextlib
import os
import sys

import torch

BAND = 64 * 1024
ALIGN = 256

_REAL_TO = torch.Tensor.to
_REAL_CLONE = torch.Tensor.clone
_HERE = os.path.abspath(__file__)
_TESTS = os.path.dirname(_HERE)
_ROOT = os.path.dirname(_TESTS)

# modules whose ``torch`` global is replaced by the proxy: the case functions and the launchers
CASE_MODULES = ("kernel_cases", "ragged_cases", "prompt_cases", "test_k1w_persist")
LAUNCHER_MODULES = tuple("lina_speech_amd." + m for m in ("kernels", "autograd", "backend", "train", "policy"))

_FACTORIES = ("empty", "zeros", "ones", "full", "tensor", "arange", "randn", "rand", "randint")
_LIKE = ("empty_like", "zeros_like", "ones_like", "full_like")


def _is_nan_filled(dtype):
    return dtype.is_floating_point or dtype.is_complex


def _site():
    """file:line (function) of the nearest caller outside this file and outside torch."""
    f = sys._getframe(1)
    while f is not None:
        fn = f.f_code.co_filename
        if os.path.abspath(fn) != _HERE and os.sep + "torch" + os.sep not in fn:
            return f"{os.path.relpath(fn, _ROOT)}:{f.f_lineno} ({f.f_code.co_name})", fn
        f = f.f_back
    return "?", ""


class GuardDamage(AssertionError):
    pass


class _Record:
    __slots__ = ("buf", "start", "nbytes", "shape", "dtype", "label", "from_launcher")


class GuardArena:
    """Hands out tensors laid out as [front band | tensor | back band] (module docstring); ``check()`` proves the bands intact."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._records = []
        self._by_storage = {}

    # ------------------------------------------------------------------ allocation
    def _alloc(self, shape, stride, dtype, label):
        shape = tuple(int(s) for s in shape)
        item = torch.empty(0, dtype=dtype).element_size()
        if stride is None:
            span = 1
            for s in shape:
                span *= s
        else:
            span = 0 if 0 in shape else 1 + sum((s - 1) * st for s, st in zip(shape, stride))
        nbytes = span * item
        raw = torch.empty(BAND + ALIGN + nbytes + BAND, dtype=torch.uint8, device=self.device)
        start = BAND + (-(raw.data_ptr() + BAND)) % ALIGN
        assert start % item == 0 and (raw.data_ptr() + start) % ALIGN == 0
        buf = raw[:start + nbytes + BAND]
        if _is_nan_filled(dtype):
            buf.fill_(0xFF)
        else:
            buf.view(dtype).fill_(1)
        t = torch.empty(0, dtype=dtype, device=self.device)
        if stride is None:
            t.set_(buf.untyped_storage(), start // item, shape)
        else:
            t.set_(buf.untyped_storage(), start // item, shape, tuple(int(s) for s in stride))
        assert t.data_ptr() == buf.data_ptr() + start or nbytes == 0
        rec = _Record()
        rec.buf, rec.start, rec.nbytes, rec.shape, rec.dtype = buf, start, nbytes, shape, dtype
        site, fn = _site()
        rec.label = label or site
        rec.from_launcher = os.path.abspath(fn).startswith(os.path.join(_ROOT, "lina-speech_amd") + os.sep)
        self._records.append(rec)
        self._by_storage[buf.untyped_storage().data_ptr()] = rec
        return t

    def empty(self, shape, dtype=torch.float32, label=None):
        """A guarded tensor whose body holds the band fill (NaN / 1)."""
        return self._alloc(shape, None, dtype, label)

    def place(self, tensor, label=None):
        """A guarded copy of ``tensor`` (same shape, dtype and values; the strides ``torch.empty_like`` would give: a dense
        permuted tensor keeps its strides, a sliced one becomes contiguous)."""
        src = tensor.detach()
        stride = torch.empty_like(src, device="meta").stride()
        out = self._alloc(src.shape, stride, src.dtype, label)
        if src.numel():
            out.copy_(src)
        return out

    # ------------------------------------------------------------------ queries
    def owns(self, tensor):
        return tensor.untyped_storage().data_ptr() in self._by_storage

    def wants(self, t):
        return (isinstance(t, torch.Tensor) and t.device.type == self.device.type and t.layout == torch.strided
                and not t.requires_grad and not t.is_inference() and not self.owns(t))

    def raw(self, tensor):
        """(uint8 buffer holding bands and tensor, byte offset of the tensor in it, the tensor's size in bytes)."""
        rec = self._by_storage[tensor.untyped_storage().data_ptr()]
        return rec.buf, rec.start, rec.nbytes

    @property
    def count(self):
        return len(self._records)

    @property
    def count_launcher(self):
        """Guarded tensors allocated from inside the package (outputs and workspaces of the launchers)."""
        return sum(r.from_launcher for r in self._records)

    # ------------------------------------------------------------------ the check
    @staticmethod
    def _bad_bytes(band, dtype):
        if _is_nan_filled(dtype):
            return band != 0xFF
        want = torch.ones(band.numel() // torch.empty(0, dtype=dtype).element_size(), dtype=dtype, device=band.device)
        return band != want.view(torch.uint8)

    def check(self):
        """Every band bit-identical to its fill, else GuardDamage naming tensor, side, first damaged byte and their number."""
        total = None
        for r in self._records:                                   # one device round trip when everything is intact
            for band in (r.buf[:r.start], r.buf[r.start + r.nbytes:]):
                n = self._bad_bytes(band, r.dtype).sum()
                total = n if total is None else total + n
        if total is None or int(total) == 0:
            return
        lines = []
        for r in self._records:
            for side, band, base in (("front", r.buf[:r.start], -r.start), ("back", r.buf[r.start + r.nbytes:], r.nbytes)):
                idx = self._bad_bytes(band, r.dtype).nonzero().flatten().cpu()
                if idx.numel():
                    lines.append(f"{side} band of tensor {r.shape} {str(r.dtype)[6:]} [{r.label}]: {idx.numel()} damaged "
                                 f"byte(s), the first at byte offset {base + int(idx[0])} relative to the tensor's first byte "
                                 f"(the tensor is {r.nbytes} bytes long)")
        raise GuardDamage("guard band damaged:\n  " + "\n  ".join(lines))


class _TorchProxy:
    """Stands in for the ``torch`` global of a module: the allocating factory functions go through the arena when they target
    the arena's device, everything else is the real ``torch``."""

    def __init__(self, arena):
        self._arena = arena
        for name in _FACTORIES:
            setattr(self, name, self._factory(getattr(torch, name), fill_body=name == "empty", like=False))
        for name in _LIKE:
            setattr(self, name, self._factory(getattr(torch, name), fill_body=name == "empty_like", like=True))

    def __getattr__(self, name):
        return getattr(torch, name)

    def _factory(self, real, fill_body, like):
        arena = self._arena

        def make(*args, **kwargs):
            out = real(*args, **kwargs)
            dev = kwargs.get("device")
            if dev is None and like and isinstance(args[0], torch.Tensor):
                dev = args[0].device
            if dev is None or "out" in kwargs or torch.device(dev).type != arena.device.type or not arena.wants(out):
                return out
            if fill_body:
                stride = None if out.is_contiguous() else out.stride()
                return arena._alloc(out.shape, stride, out.dtype, None)
            return arena.place(out)
        make.__name__ = real.__name__
        return make


@contextlib.contextmanager
def guarded(monkeypatch, device):
    """Route the tensors of the case functions and of the launchers into a fresh GuardArena (module docstring) while the block
    runs; yields the arena.  Everything is put back by ``monkeypatch`` (at the end of the block and of the test)."""
    import importlib
    from lina_speech_amd import ops
    ops.clear_workspaces()          # cached scratch (segment states of K2 / K2b, padded MLP weights) is allocated anew: guarded
    arena = GuardArena(device)
    proxy = _TorchProxy(arena)

    def to(self, *args, **kwargs):
        out = _REAL_TO(self, *args, **kwargs)
        if (len(args) == 1 and not kwargs and isinstance(args[0], (str, torch.device))
                and torch.device(args[0]).type == arena.device.type and arena.wants(out)):
            return arena.place(out)
        return out

    def clone(self, *args, **kwargs):
        if not args and not kwargs and not self.requires_grad and not self.is_inference() and arena.owns(self):
            return arena.place(self)
        return _REAL_CLONE(self, *args, **kwargs)

    with monkeypatch.context() as mp:
        for name in CASE_MODULES + LAUNCHER_MODULES:
            mod = importlib.import_module(name)
            if getattr(mod, "torch", None) is torch:
                mp.setattr(mod, "torch", proxy)
        real_pack = ops.pack_rows

        def pack_rows(t, out=None):
            p = real_pack(t, out)
            return arena.place(p) if out is None and arena.wants(p) else p
        mp.setattr(ops, "pack_rows", pack_rows)
        mp.setattr(torch.Tensor, "to", to)
        mp.setattr(torch.Tensor, "clone", clone)
        try:
            yield arena
        finally:
            ops.clear_workspaces()  # nothing of the arena stays cached in the package
