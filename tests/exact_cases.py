"""Exact-integer kernel checks: bit-exact comparisons for the paths the tolerance tests cannot pin down.

Every kernel checked here is multilinear in its data once the gates are zero.  Fed with operands from {-1, 0, +1} (times a
power of two where the op takes a scale), sparse enough that every partial sum stays a small integer, every product, every
partial sum IN ANY ORDER and every bf16 rounding of an intermediate is exact: the kernel must reproduce the fp64 oracle,
rounded ONCE to the output dtype, bit for bit.  A dropped, doubled or misplaced element changes a result by at least one
unit, which the 2e-2-of-the-maximum bound of ``kernel_cases.assert_close`` lets through (``test_exact_emu.py`` shows that
on a K = 1376 projection).  Summation order, MFMA accumulation order and split-K are irrelevant, so the CPU emulator and the
device must hit the same bits.

What makes the claim true is asserted in every case, on the ORACLE's side only (``assert_exact_range``): every value a
kernel may hold in bf16 -- the inputs, the state at every token, the scores tril(q k^T), the backward's tril(do v^T) and
state gradient, every bf16 output before its single rounding -- is an integer multiple of the scale of magnitude
<= 256 x scale, and every fp32 accumulation stays below 2^24.

Gates: all gates are exactly 0 (every decay is exp(0) = 1).  Reset gates stay with the tolerance tests: inside a chunk the
kernels rescale through exp(b) exp(-b) pairs that are not exact reciprocals for b != 0, so a reset pattern is legitimately
inexact.  Not linear, and therefore out of reach here: the LayerNorm fold, SwiGLU, the in-projection prologue, softmax and
norm kernels, sampling, AdamW.

The sign of a zero carries no information about a lost term (0 * -1 = -0 where a sum of terms gives +0): zeros are
compared as +0, everything else through an integer view of the bits.

``dev`` = "cpu" (ops bound to the wave64 emulator) or "cuda", as in ``kernel_cases``.
"""
import functools
import os

import torch
import torch.nn.functional as F

import kernel_cases as KC
from kernel_cases import LibCalls
from lina_speech_amd import ops
from oracle import gla_oracle as O

F64 = torch.float64
BF16, F32 = torch.bfloat16, torch.float32
DENSITY = 0.25                      # at 1/2 the K2 output leaves the bf16-exact range (|o| / scale > 256 at T = 300)
BF16_LIMIT = 256.0                  # integers up to 2^8 are bf16 values
F32_LIMIT = float(2 ** 24)


# ----------------------------------------------------------------------------- helpers
def ternary(shape, density, gen, dtype, scale=1.0):
    """+-scale with probability ``density`` (half each), otherwise 0; ``scale`` a power of two."""
    u = torch.rand(*shape, generator=gen)
    t = torch.where(u < density / 2, -1.0, torch.where(u < density, 1.0, 0.0)) * scale
    return t.to(dtype)


def _bits(t):
    t = (t.detach().cpu() + 0.0).contiguous()              # -0 -> +0
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_exact(got, ref64, what):
    """``got`` == the exact value ``ref64`` rounded once (to nearest) to got's dtype, bit for bit."""
    ref64 = ref64.detach().cpu()
    assert ref64.dtype == F64, f"{what}: the reference must be fp64"
    assert tuple(got.shape) == tuple(ref64.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    want = ref64.to(got.dtype)
    diff = _bits(got) != _bits(want)
    n = int(diff.sum())
    KC.record_parity(what, n, 0)
    if n:
        g, idx = got.detach().cpu(), diff.nonzero()[:8].tolist()
        shown = ", ".join(f"{tuple(i)}: got {float(g[tuple(i)])!r} want {float(want[tuple(i)])!r}" for i in idx)
        raise AssertionError(f"{what}: {n} of {diff.numel()} elements differ from the exact result; first: {shown}")


def assert_exact_range(ref64_tensors, limit=BF16_LIMIT, unit=1.0):
    """The precondition of exactness, on fp64 oracle values only: every element of every tensor in ``ref64_tensors``
    ({name: tensor}) is an integer multiple of ``unit`` with magnitude <= limit * unit.  ``limit`` = 256 for what a kernel may
    hold in bf16, 2^24 for fp32 accumulations."""
    for name, t in ref64_tensors.items():
        if t is None:
            continue
        assert t.dtype == F64, f"range precondition on {name}: computed in {t.dtype}, not fp64"
        m = t.detach() / unit
        assert torch.equal(m, m.round()), f"range precondition: {name} is not a multiple of {unit}"
        top = float(m.abs().max()) if m.numel() else 0.0
        assert top <= limit, f"range precondition: max|{name}| = {top:g} x {unit} exceeds {limit:g} x {unit}"


class _few_threads:
    """A long python loop of tiny ops: a machine-wide thread pool only adds wake-up cost (as kernel_cases.oracle_gla)."""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(min(self.n, 8))

    def __exit__(self, *exc):
        torch.set_num_threads(self.n)
        return False


# ----------------------------------------------------------------------------- GLA: inputs and fp64 references (cached)
@functools.lru_cache(maxsize=6)
def _gla_case(B, H, T, Dk, Dv, seed, density=DENSITY):
    """Ternary q, k, v (laid out [B,T,H*D] and seen head-first, as the projections arrive), h0, d_o, d_ht: fp64, CPU."""
    g = torch.Generator().manual_seed(1000 + seed)
    heads = lambda x: x.view(B, T, H, -1).transpose(1, 2)
    q, k = (heads(ternary((B, T, H * Dk), density, g, F64)) for _ in range(2))
    v = heads(ternary((B, T, H * Dv), density, g, F64))
    h0 = ternary((B, H, Dk, Dv), density, g, F64)
    d_o = heads(ternary((B, T, H * Dv), density, g, F64))
    # the gradient of the final state in units of the scale: dk = v dS^T sums ~Dv/16 entries of it, at +-1 that alone is
    # 16 (Dk = 256) x 16 terms x the tail of the distribution > 256 scale units (measured 290 .. 383 at T = 40 .. 70)
    d_ht = ternary((B, H, Dk, Dv), density, g, F64, scale=_pow2_scale(Dk))
    return dict(q=q, k=k, v=v, h0=h0, d_o=d_o, d_ht=d_ht)


def _pow2_scale(Dk):
    """Dk ** -0.5 where that is a power of two (1/8 at 64, 1/16 at 256); 1/8 for Dk = 128, passed explicitly."""
    return {64: 0.125, 128: 0.125, 256: 0.0625}[Dk]


@functools.lru_cache(maxsize=12)
def _gla_fwd_ref(B, H, T, Dk, Dv, seed, with_h0, density=DENSITY):
    """(o, S_T) of the fp64 recurrent oracle at zero gates, with the forward range preconditions asserted: inputs, the state
    at EVERY token, the scores tril(q k^T), o / scale."""
    c = _gla_case(B, H, T, Dk, Dv, seed, density)
    q, k, v = c["q"], c["k"], c["v"]
    h0 = c["h0"] if with_h0 else None
    scale = _pow2_scale(Dk)
    with _few_threads():
        o, S = O.naive_recurrent_gla(q, k, v, torch.zeros_like(q), initial_state=h0, output_final_state=True, scale=scale,
                                     compute_dtype=F64)
        Srun = torch.zeros(B, H, Dk, Dv, dtype=F64) if h0 is None else h0.clone()
        smax = Srun.abs().max().clone()
        for t in range(T):
            Srun += k[:, :, t].unsqueeze(-1) * v[:, :, t].unsqueeze(-2)
            smax = torch.maximum(smax, Srun.abs().max())
    assert torch.equal(Srun, S), "the oracle's final state is not the plain sum of k_t v_t^T"
    scores = torch.tril(q @ k.transpose(-1, -2))
    assert_exact_range({"q": q, "k": k, "v": v, "h0": h0, "max_t |S_t|": smax.reshape(1), "tril(q k^T)": scores, "S_T": S})
    assert_exact_range({"o": o}, unit=scale)
    return o, S


def _oracle_grads(q, k, v, h0, d_o, d_ht, scale, seg=64):
    """Gradients of sum(o d_o) + sum(S_T d_ht) w.r.t. q, k, v, g, h0: fp64 torch autograd through
    oracle.naive_recurrent_gla at zero gates, run segment by segment from the last to the first with the state gradient
    handed down (the same numbers as one pass over all T steps, at a fraction of its memory)."""
    B, H, T, Dk = q.shape
    Dv = v.shape[-1]
    gk = torch.zeros_like(q)
    S = torch.zeros(B, H, Dk, Dv, dtype=F64) if h0 is None else h0.clone()
    starts = []
    with torch.no_grad():
        for t0 in range(0, T, seg):
            starts.append(S)
            sl = slice(t0, min(T, t0 + seg))
            _, S = O.naive_recurrent_gla(q[:, :, sl], k[:, :, sl], v[:, :, sl], gk[:, :, sl], initial_state=S,
                                         output_final_state=True, scale=scale, compute_dtype=F64)
    dS = torch.zeros_like(S) if d_ht is None else d_ht.clone()
    grads = [torch.empty_like(x) for x in (q, k, v, gk)]
    for i in reversed(range(len(starts))):
        sl = slice(i * seg, min(T, (i + 1) * seg))
        leaves = [x[:, :, sl].clone().requires_grad_(True) for x in (q, k, v, gk)]
        s_in = starts[i].clone().requires_grad_(True)
        o, s_out = O.naive_recurrent_gla(*leaves, initial_state=s_in, output_final_state=True, scale=scale, compute_dtype=F64)
        ((o * d_o[:, :, sl]).sum() + (s_out * dS).sum()).backward()
        for gsum, leaf in zip(grads, leaves):
            gsum[:, :, sl] = leaf.grad
        dS = s_in.grad
    return dict(dq=grads[0], dk=grads[1], dv=grads[2], dg=grads[3], dh0=dS)


@functools.lru_cache(maxsize=8)
def _gla_bwd_ref(B, H, T, Dk, Dv, seed, with_h0, with_dht, density=DENSITY):
    """fp64 gradients with the backward's range preconditions asserted: d_o, d_ht, tril(do v^T), the state gradient at every
    token, dq / dk / dv (bf16 outputs: <= 256 x scale), dg and dh0 (fp32 accumulations: < 2^24)."""
    c = _gla_case(B, H, T, Dk, Dv, seed, density)
    q, k, v, d_o = c["q"], c["k"], c["v"], c["d_o"]
    h0 = c["h0"] if with_h0 else None
    d_ht = c["d_ht"] if with_dht else None
    scale = _pow2_scale(Dk)
    with _few_threads():
        r = _oracle_grads(q, k, v, h0, d_o, d_ht, scale)
        dS = torch.zeros(B, H, Dk, Dv, dtype=F64) if d_ht is None else d_ht.clone()
        dmax = dS.abs().max().clone()
        for t in reversed(range(T)):
            dS += scale * q[:, :, t].unsqueeze(-1) * d_o[:, :, t].unsqueeze(-2)
            dmax = torch.maximum(dmax, dS.abs().max())
    assert torch.equal(dS, r["dh0"]), "the oracle's dh0 is not the plain sum of the state gradient"
    assert_exact_range({"d_o": d_o, "tril(do v^T)": torch.tril(d_o @ v.transpose(-1, -2))})
    assert_exact_range({"d_ht": d_ht, "max_t |dS_t|": dmax.reshape(1), "dq": r["dq"], "dk": r["dk"], "dv": r["dv"]}, unit=scale)
    assert_exact_range({"dg": r["dg"], "dh0": r["dh0"]}, limit=F32_LIMIT, unit=scale)
    return r


def _dev_inputs(c, dtype, dev, with_h0):
    q, k, v = (c[n].to(dtype).to(dev) for n in ("q", "k", "v"))
    h0 = c["h0"].float().to(dev) if with_h0 else None
    return q, k, v, h0


# ----------------------------------------------------------------------------- K1
def check_exact_recurrent(dev, B, H, T, Dk, Dv, dtype, seed=1):
    """K1 ``fused_recurrent_gla``: o and the final state with h0, without h0, in the in-place state form; bf16 with bf16 and
    with fp32 (zero) gates."""
    c = _gla_case(B, H, T, Dk, Dv, seed)
    scale = _pow2_scale(Dk)
    for with_h0 in (True, False):
        ro, rS = _gla_fwd_ref(B, H, T, Dk, Dv, seed, with_h0)
        q, k, v, h0 = _dev_inputs(c, dtype, dev, with_h0)
        for gdt in ((dtype, F32) if dtype == BF16 else (F32,)):
            gk = torch.zeros_like(q, dtype=gdt)
            o, S = ops.fused_recurrent_gla(q, k, v, gk, scale=scale, initial_state=h0, output_final_state=True)
            assert o.dtype == dtype and S.dtype == F32
            tag = f"K1 {Dk}x{Dv} T{T} h0={with_h0} gates {gdt}"
            assert_exact(o, ro, f"exact {tag}: o")
            assert_exact(S, rS, f"exact {tag}: state")
        if with_h0:
            h_in = h0.clone()
            o3, S3 = ops.fused_recurrent_gla(q, k, v, torch.zeros_like(q), scale=scale, initial_state=h_in,
                                             output_final_state=True, inplace_state=True)
            assert S3.data_ptr() == h_in.data_ptr()
            assert_exact(o3, ro, f"exact K1 {Dk}x{Dv} T{T} in place: o")
            assert_exact(S3, rS, f"exact K1 {Dk}x{Dv} T{T} in place: state")


# ----------------------------------------------------------------------------- K1d
def check_exact_decode_update(dev, B, H, Dk, Dv, dtype, steps=3, seed=2):
    """K1d ``gla_decode_update`` and K1d + K5 ``gla_decode_update_norm`` over ``steps`` consecutive steps: the state after
    each step and the sum over the Dk/64 row blocks of ``o_part`` (= scale q S) are exact; og (through the RMS norm) finite."""
    g = torch.Generator().manual_seed(2000 + seed)
    scale, NP = _pow2_scale(Dk), Dk // 64
    S_ref = ternary((B, H, Dk, Dv), DENSITY, g, F64)
    S_a, S_b = S_ref.float().to(dev), S_ref.float().to(dev)
    w = torch.ones(Dv, dtype=dtype, device=dev)
    counters = torch.zeros(B * H, dtype=torch.int32, device=dev)
    for t in range(steps):
        q64, k64 = (ternary((B, H, Dk), DENSITY, g, F64) for _ in range(2))
        v64, gate64 = (ternary((B, H, Dv), DENSITY, g, F64) for _ in range(2))
        S_ref = S_ref + k64.unsqueeze(-1) * v64.unsqueeze(-2)
        o_ref = torch.einsum("bhk,bhkv->bhv", q64 * scale, S_ref)
        assert_exact_range({"q": q64, "k": k64, "v": v64, "S": S_ref})
        assert_exact_range({"o": o_ref}, unit=scale)
        q, k, v, gate = (x.to(dtype).to(dev) for x in (q64, k64, v64, gate64))
        gk = torch.zeros(B, H, Dk, device=dev)
        op_a = torch.full((NP, B, H, Dv), float("nan"), device=dev)
        ops.gla_decode_update(q, k, v, gk, op_a, S_a, scale=scale)
        assert_exact(S_a, S_ref, f"exact K1d {Dk}x{Dv} {dtype} step {t}: state")
        assert_exact(op_a.sum(0), o_ref, f"exact K1d {Dk}x{Dv} {dtype} step {t}: sum of o_part")
        op_b = torch.full((NP, B, H, Dv), float("nan"), device=dev)
        og = torch.full((B, H, Dv), float("nan"), dtype=dtype, device=dev)
        ops.gla_decode_update_norm(q, k, v, gk, op_b, S_b, gate, w, og, counters, 1e-5, scale=scale)
        assert_exact(S_b, S_ref, f"exact K1d+K5 {Dk}x{Dv} {dtype} step {t}: state")
        assert_exact(op_b.sum(0), o_ref, f"exact K1d+K5 {Dk}x{Dv} {dtype} step {t}: sum of o_part")
        assert torch.isfinite(og.float()).all() and int(counters.abs().sum()) == 0


# ----------------------------------------------------------------------------- K1w
def check_exact_decode_window(dev, B, H, Dk, Dv, dtype, state_dtype, window, n_wg, seed=3):
    """K1w ``gla_decode_window`` (``n_wg`` = 0: one workgroup per head; > 0: the persistent kernel) over 2 window + 3 steps:
    the history rows written so far (hist_k = k_s, hist_v = v_s, hist_c = the cumulative gate = 0; window > 1), the state
    after every completed window and after the flush.  A bf16 state is exact too (integers <= 256).  og passes through the RMS
    norm: finite only."""
    g = torch.Generator().manual_seed(3000 + seed)
    scale, n_steps, origin0 = _pow2_scale(Dk), 2 * window + 3, 5
    S_ref = ternary((B, H, Dk, Dv), DENSITY, g, F64)
    S = S_ref.to(state_dtype).to(dev)
    hk, hc = (torch.zeros(window, B * H, Dk, device=dev) for _ in range(2))
    hv = torch.zeros(window, B * H, Dv, device=dev)
    w = torch.ones(Dv, dtype=dtype, device=dev)
    counters = torch.zeros(B * H, dtype=torch.int32, device=dev)
    o_x = torch.zeros(B * H * Dv, device=dev) if Dv > 256 else None
    origin = torch.full((1,), origin0, dtype=torch.int64, device=dev)
    tag = f"exact K1w {Dk}x{Dv} {dtype} state {state_dtype} window {window} n_wg {n_wg}"
    in_window = []
    for t in range(n_steps):
        q64, k64 = (ternary((B, H, Dk), DENSITY, g, F64) for _ in range(2))
        v64, gate64 = (ternary((B, H, Dv), DENSITY, g, F64) for _ in range(2))
        S_ref = S_ref + k64.unsqueeze(-1) * v64.unsqueeze(-2)
        assert_exact_range({"q": q64, "k": k64, "v": v64, "S": S_ref})
        assert_exact_range({"o": torch.einsum("bhk,bhkv->bhv", q64 * scale, S_ref)}, unit=scale)
        q, k, v, gate = (x.to(dtype).to(dev) for x in (q64, k64, v64, gate64))
        og = torch.full((B, H, Dv), float("nan"), dtype=dtype, device=dev)
        step = torch.full((1,), origin0 + t, dtype=torch.int64, device=dev)
        ops.gla_decode_window(q, k, v, torch.zeros(B, H, Dk, device=dev), S, gate, w, og, hk, hc, hv, step, origin, window,
                              1e-5, scale=scale, o_exchange=o_x, counters=counters, n_wg=n_wg)
        assert torch.isfinite(og.float()).all(), f"{tag}: og at step {t}"
        assert int(counters.abs().sum()) == 0
        if t % window == 0:
            in_window = []
        in_window.append((k64, v64))
        if window > 1:
            p = len(in_window)
            assert_exact(hk[:p], torch.stack([a for a, _ in in_window]).view(p, B * H, Dk), f"{tag}: hist_k")
            assert_exact(hv[:p], torch.stack([b for _, b in in_window]).view(p, B * H, Dv), f"{tag}: hist_v")
            assert_exact(hc[:p], torch.zeros(p, B * H, Dk, dtype=F64), f"{tag}: hist_c")
        if (t + 1) % window == 0:
            assert_exact(S, S_ref, f"{tag}: state after a window")
    ops.gla_decode_window_flush(S, hk, hc, hv, n_steps % window)
    assert_exact(S, S_ref, f"{tag}: flushed state")


# ----------------------------------------------------------------------------- K2
def _nseg_launched(calls):
    return [int(a[KC._FWD_SEG_NSEG]) for a in calls.of("lina_gla_chunk_fwd_seg")]


def check_exact_chunk(dev, B, H, T, Dk, Dv, dtype, nsegs=(None,), seed=4, fns=("chunk_gla", "fused_chunk_gla")):
    """K2 forward through ``ops.chunk_gla`` / ``ops.fused_chunk_gla``: o and the final state with and without h0.  ``nsegs``:
    segment counts to run (``chunk_gla`` only; None = the launch policy's); all of them must give the same bits, and every
    one the oracle's."""
    c = _gla_case(B, H, T, Dk, Dv, seed)
    scale = _pow2_scale(Dk)
    for with_h0 in (True, False):
        ro, rS = _gla_fwd_ref(B, H, T, Dk, Dv, seed, with_h0)
        q, k, v, h0 = _dev_inputs(c, dtype, dev, with_h0)
        gk = torch.zeros_like(q)
        outs = {}
        for name in fns:
            for ns in (nsegs if name == "chunk_gla" else (None,)):
                kw = {} if name != "chunk_gla" else {"nseg": ns}
                with LibCalls() as calls:
                    o, S = getattr(ops, name)(q, k, v, gk, scale=scale, initial_state=h0, output_final_state=True, **kw)
                if ns is not None and ns > 1:
                    assert _nseg_launched(calls) == [ns], f"segment-parallel K2 launches {_nseg_launched(calls)}, wanted {ns}"
                    assert not calls.of("lina_gla_chunk_fwd"), "the segment-parallel kernel refused the layout"
                assert o.dtype == dtype and S.dtype == F32
                tag = f"exact K2 {name} {Dk}x{Dv} H{H} T{T} {dtype} nseg={ns} h0={with_h0}"
                assert_exact(o, ro, f"{tag}: o")
                assert_exact(S, rS, f"{tag}: state")
                outs[(name, ns)] = (o, S)
        first = next(iter(outs.values()))
        for key, (o, S) in outs.items():
            assert torch.equal(_bits(o), _bits(first[0])) and torch.equal(_bits(S), _bits(first[1])), f"{key} differs in bits"


def check_exact_chunk_dv512(dev, monkeypatch, B, H, T, seed=5):
    """256 x 512 heads (gla_chunk_full.hip NCB = 2): both value column blocks in one launch and one launch per block, each
    against the oracle and bit-equal to each other."""
    res = []
    for one in (True, False):
        monkeypatch.setattr(ops.POLICY, "dv512_one_launch", one)
        with LibCalls() as calls:
            check_exact_chunk(dev, B, H, T, 256, 512, BF16, nsegs=(1,), seed=seed, fns=("chunk_gla",))
        n = len(calls.of("lina_gla_chunk_fwd"))
        res.append(n)
    assert res[1] == 2 * res[0], f"one launch / two launches made {res} calls of lina_gla_chunk_fwd"


def check_exact_chunk_simple(dev, B, H, T, Dk, Dv, dtype, seed=6):
    """``ops.chunk_simple_gla`` with zero head gates [B,H,T] (fp32): the same oracle values."""
    c = _gla_case(B, H, T, Dk, Dv, seed)
    scale = _pow2_scale(Dk)
    for with_h0 in (True, False):
        ro, rS = _gla_fwd_ref(B, H, T, Dk, Dv, seed, with_h0)
        q, k, v, h0 = _dev_inputs(c, dtype, dev, with_h0)
        g = torch.zeros(B, H, T, device=dev)
        o, S = ops.chunk_simple_gla(q, k, v, g, scale=scale, initial_state=h0, output_final_state=True)
        assert o.dtype == dtype and S.dtype == F32
        assert_exact(o, ro, f"exact simple-GLA {Dk}x{Dv} T{T} {dtype} h0={with_h0}: o")
        assert_exact(S, rS, f"exact simple-GLA {Dk}x{Dv} T{T} {dtype} h0={with_h0}: state")


# ----------------------------------------------------------------------------- K2b
def _dv_block_preconditions(B, H, T, Dk, Dv, seed, with_h0, with_dht):
    """Dv = 2 Dk on the column-block route (kernels.gla_chunk_bwd, ``m > 1``): every block's dq, dk and dg is ROUNDED TO
    bf16 before the blocks are added (``gq.float()`` of a bf16 tensor), so each block's own gradients must be bf16 values --
    computed here per block through the fp64 oracle."""
    c = _gla_case(B, H, T, Dk, Dv, seed)
    scale = _pow2_scale(Dk)
    for j in range(Dv // Dk):
        cols = slice(j * Dk, (j + 1) * Dk)
        part = lambda t: t[..., cols].contiguous()
        with _few_threads():
            r = _oracle_grads(c["q"], c["k"], part(c["v"]), part(c["h0"]) if with_h0 else None, part(c["d_o"]),
                              part(c["d_ht"]) if with_dht else None, scale)
        assert_exact_range({f"block {j} {n}": r[n] for n in ("dq", "dk", "dg")}, unit=scale)


def check_exact_chunk_bwd(dev, B, H, T, Dk, Dv, dtype, nseg=None, path=None, with_h0=True, with_dht=True, seed=7,
                          direct=True, autograd=True):
    """K2b: dq, dk, dv, dg, dh0 from ternary d_o and d_ht, through ``ops.gla_chunk_bwd`` (``path``: "full" = the three
    sweeps of the full-head kernel, "sweeps" = the generic kernel) and through autograd of ``ops.chunk_gla`` (which also
    re-checks o and the final state), against fp64 autograd through the recurrent oracle.  dg is an integer multiple of the
    scale beyond 256: correctly rounded to bf16 by ``.to(bf16)``, it needs the fp32 bound only."""
    c = _gla_case(B, H, T, Dk, Dv, seed)
    scale = _pow2_scale(Dk)
    ref = _gla_bwd_ref(B, H, T, Dk, Dv, seed, with_h0, with_dht)
    ro, rS = _gla_fwd_ref(B, H, T, Dk, Dv, seed, with_h0)
    if dtype == BF16 and Dk == 256 and Dv > Dk:
        _dv_block_preconditions(B, H, T, Dk, Dv, seed, with_h0, with_dht)
    q, k, v, h0 = _dev_inputs(c, dtype, dev, with_h0)
    gk = torch.zeros_like(q)
    d_o = c["d_o"].to(dtype).to(dev)
    d_ht = c["d_ht"].float().to(dev) if with_dht else None
    tag = f"exact K2b {Dk}x{Dv} H{H} T{T} {dtype} nseg={nseg} path={path} h0={with_h0} dht={with_dht}"

    def compare(got, how):
        for name, a in zip(("dq", "dk", "dv", "dg", "dh0"), got):
            if name == "dh0" and not with_h0:
                continue
            assert a is not None, f"{tag} {how}: no {name}"
            assert_exact(a, ref[name], f"{tag} {how}: {name}")

    if direct:
        ht = rS.float().to(dev) if with_dht else None              # the oracle's final state: an INPUT of the backward
        with LibCalls() as calls:
            got = ops.gla_chunk_bwd(q, k, v, gk, d_o, scale, h0, ht, d_ht, need_dh0=with_h0, nseg=nseg, path=path)
        if path == "full" and dtype == BF16:
            assert calls.of("lina_gla_chunk_bwd_full") and not calls.of("lina_gla_chunk_bwd"), "not the full-head sweeps"
        if path == "sweeps":
            assert calls.of("lina_gla_chunk_bwd") and not calls.of("lina_gla_chunk_bwd_full"), "not the generic kernel"
        compare(got, "direct")
    if autograd:
        leaves = [x.detach().clone().requires_grad_(True) for x in (q, k, v, gk)]
        lh0 = None if h0 is None else h0.detach().clone().requires_grad_(True)
        o, S = ops.chunk_gla(*leaves, scale=scale, initial_state=lh0, output_final_state=with_dht, nseg=nseg)
        assert_exact(o, ro, f"{tag} autograd: o")
        loss = (o.float() * d_o.float()).sum()
        if with_dht:
            assert_exact(S, rS, f"{tag} autograd: state")
            loss = loss + (S * d_ht).sum()
        loss.backward()
        compare([x.grad for x in leaves] + [None if lh0 is None else lh0.grad], "autograd")


# ----------------------------------------------------------------------------- projections
def _linear_case(M, N, K, dtype, dev, bias, resid, seed=8):
    g = torch.Generator().manual_seed(4000 + seed)
    a64, w64 = ternary((M, K), DENSITY, g, F64), ternary((N, K), DENSITY, g, F64)
    b64 = ternary((N,), DENSITY, g, F64) if bias else None
    r64 = ternary((M, N), DENSITY, g, F64) if resid else None
    y64 = a64 @ w64.t()
    assert_exact_range({"a": a64, "w": w64, "bias": b64, "resid": r64, "a w^T": y64})
    if bias:
        y64 = y64 + b64
    if resid:
        y64 = y64 + r64
    assert_exact_range({"y": y64})
    a, w = a64.to(dtype).to(dev), w64.to(dtype).to(dev)
    b = None if b64 is None else b64.float().to(dev)
    r = None if r64 is None else r64.to(dtype).to(dev)
    return a, w, b, r, y64


def check_exact_linear_skinny(dev, M, N, K, dtype, bias=False, resid=False):
    """``ops.linear_skinny`` (no LayerNorm fold, no SwiGLU: those are not linear) with ternary a, w, bias and residual; with a
    residual also the in-place form (out aliases resid)."""
    a, w, b, r, y64 = _linear_case(M, N, K, dtype, dev, bias, resid)
    tag = f"exact linear_skinny M{M} N{N} K{K} {dtype}"
    out = ops.linear_skinny(a, w, None, b, resid=r, n_out=N)
    assert out.shape == (M, N) and out.dtype == dtype
    assert_exact(out, y64, tag)
    if resid:
        r2 = r.clone()
        ops.linear_skinny(a, w, None, b, resid=r2, out=r2, n_out=N)
        assert_exact(r2, y64, f"{tag} in place")


def _packed_run(a_p, w_p, M, N, K, Np, b, r, dtype, dev):
    out = torch.full((M, N), float("nan"), dtype=dtype, device=dev)
    out_p = torch.zeros(ops.packed_numel(M, Np), dtype=dtype, device=dev)
    ops.linear_skinny_packed(a_p, w_p, M, N, K, None, b, resid=r, out=out, out_packed=out_p, out_packed_width=Np)
    x_p = None
    if r is not None:                     # the residual stream held only in packed form, updated in place
        rp = torch.zeros(M, Np, dtype=dtype, device=dev)
        rp[:, :N] = r
        x_p = ops.pack_rows(rp)
        ops.linear_skinny_packed(a_p, w_p, M, N, K, None, b, resid=x_p, out_packed=x_p, out_packed_width=Np)
    return out, out_p, x_p


def _check_packed_outputs(outs, M, N, Np, y64, tag):
    out, out_p, x_p = outs
    assert_exact(out, y64, f"{tag}: row-major output")
    assert_exact(ops.unpack_rows(out_p, M, Np)[:, :N], y64, f"{tag}: packed copy")
    if N < Np:
        assert float(ops.unpack_rows(out_p, M, Np)[:, N:].float().abs().max()) == 0.0, f"{tag}: packed pad columns"
    if x_p is not None:
        assert_exact(ops.unpack_rows(x_p, M, Np)[:, :N], y64, f"{tag}: in-place packed residual")


def check_exact_linear_skinny_packed(dev, M, N, K, dtype, bias=False, resid=False):
    """``ops.linear_skinny_packed`` (fragment-major a and w): the row-major output, the packed copy, the in-place packed
    residual form, and row-major inputs with a packed output copy -- each against the fp64 product."""
    a, w, b, r, y64 = _linear_case(M, N, K, dtype, dev, bias, resid, seed=9)
    kq = 32 if dtype == BF16 else 16
    Np = (N + kq - 1) // kq * kq
    tag = f"exact linear_skinny_packed M{M} N{N} K{K} {dtype}"
    _check_packed_outputs(_packed_run(ops.pack_rows(a), ops.pack_rows(w), M, N, K, Np, b, r, dtype, dev), M, N, Np, y64, tag)
    out_p2 = torch.zeros(ops.packed_numel(M, Np), dtype=dtype, device=dev)
    out2 = ops.linear_skinny(a, w, None, b, resid=r, n_out=N, out_packed=out_p2, out_packed_width=Np)
    assert_exact(out2, y64, f"{tag}: row-major inputs, row-major output")
    assert_exact(ops.unpack_rows(out_p2, M, Np)[:, :N], y64, f"{tag}: row-major inputs, packed copy")


def check_exact_linear_tall(dev, M, N, K, dtype, variant, bias=False, resid=False):
    """The tall tiling (LINA_TALL=1, LINA_TALL_V = ``variant``; set and restored as kernel_cases.check_linear_tall does)
    against the fp64 product, and ``torch.equal`` to the skinny kernel: with exact sums there is no rounding between them."""
    a, w, b, r, y64 = _linear_case(M, N, K, dtype, dev, bias, resid, seed=10)
    kq = 32 if dtype == BF16 else 16
    Np = (N + kq - 1) // kq * kq
    a_p, w_p = ops.pack_rows(a), ops.pack_rows(w)
    prev, prev_v = os.environ.get("LINA_TALL"), os.environ.get("LINA_TALL_V")
    try:
        os.environ["LINA_TALL_V"] = str(variant)
        os.environ["LINA_TALL"] = "0"
        skinny = _packed_run(a_p, w_p, M, N, K, Np, b, r, dtype, dev)
        os.environ["LINA_TALL"] = "1"
        tall = _packed_run(a_p, w_p, M, N, K, Np, b, r, dtype, dev)
    finally:
        for name, old in (("LINA_TALL", prev), ("LINA_TALL_V", prev_v)):
            if old is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = old
    tag = f"exact linear tall (variant {variant}) M{M} N{N} K{K} {dtype}"
    _check_packed_outputs(tall, M, N, Np, y64, tag)
    _check_packed_outputs(skinny, M, N, Np, y64, f"{tag}, skinny tiling")
    assert torch.equal(tall[0], skinny[0]) and torch.equal(tall[1], skinny[1]), f"{tag}: tall != skinny"


def check_exact_weighted_rows_add(dev, B, Tn, d, dtype, seed=11):
    """``ops.weighted_rows_add`` (row-major and ``x_packed``): x += sum_t att[t] vv[t] with attention weights n/64,
    n = 0..7, and ternary vv and x.  Everything is a multiple of 1/64; |x| <= 256/64 asserted."""
    g = torch.Generator().manual_seed(5000 + seed)
    unit = 1.0 / 64
    Tp = (Tn + 31) // 32 * 32
    att64 = torch.zeros(B, Tp, dtype=F64)
    att64[:, :Tn] = torch.randint(0, 8, (B, Tn), generator=g).to(F64) * unit
    vv64, x64 = ternary((B, Tn, d), DENSITY, g, F64), ternary((B, d), DENSITY, g, F64)
    acc = torch.einsum("bt,btd->bd", att64[:, :Tn], vv64)
    y64 = x64 + acc
    assert_exact_range({"att": att64, "sum": acc, "x + sum": y64}, unit=unit)
    assert_exact_range({"vv": vv64, "x": x64})
    attc, vv = att64.to(dtype).to(dev), vv64.to(dtype).to(dev)
    x = x64.to(dtype).to(dev)
    ops.weighted_rows_add(attc, vv, x)
    assert_exact(x, y64, f"exact weighted_rows_add B{B} Tn{Tn} d{d} {dtype}")
    x0 = x64.to(dtype).to(dev)
    x_p = ops.pack_rows(x0)
    ops.weighted_rows_add(attc, vv, x0, x_packed=x_p)
    assert_exact(ops.unpack_rows(x_p, B, d), y64, f"exact weighted_rows_add (packed) B{B} Tn{Tn} d{d} {dtype}")
    assert_exact(x0, x64, "exact weighted_rows_add (packed): the row-major x is not touched")


# ----------------------------------------------------------------------------- sums and gathers
def check_exact_embed_sum(dev, dtype, Q=4, B=3, n=5, n_emb=37, d=64, seed=12):
    g = torch.Generator().manual_seed(6000 + seed)
    t64 = ternary((Q, n_emb, d), DENSITY, g, F64)
    idx = torch.randint(0, n_emb, (Q, B, n), generator=g)
    ref = O.embed_sum(t64, idx)
    assert_exact_range({"table": t64, "sum": ref})
    out = ops.embed_sum(t64.to(dtype).to(dev), idx.to(dev))
    assert out.shape == (B, n, d) and out.dtype == dtype
    assert_exact(out, ref, f"exact embed_sum Q{Q} {dtype}")


def check_exact_sums(dev):
    """``ops._sum_partials`` / ``_sum_partials2`` / ``column_sum`` / ``_sum_vector`` at the sizes of
    kernel_cases.check_sum_partials / check_column_sum, on ternary data: integer sums, far below 2^24 (and <= 256 where the
    result is bf16)."""
    g = torch.Generator().manual_seed(7000)
    for P, shape in ((1, (8,)), (7, (40, 5)), (37, (256,)), (300, (1024, 5)), (513, (260,)), (16, (3,)), (1024, (256,)),
                     (130, (2816,)), (64, (3072, 5)), (256, (1024, 17)), (1025, (1024,))):
        p64 = ternary((P, *shape), DENSITY, g, F64)
        ref = p64.sum(0)
        assert_exact_range({"partial sums": ref}, limit=F32_LIMIT)
        got = ops._sum_partials(p64.float().to(dev))
        assert got.shape == shape and got.dtype == F32
        assert_exact(got, ref, f"exact K13 P={P} {shape}")
    p64 = ternary((2, 77, 512), DENSITY, g, F64)
    assert_exact(ops._sum_partials2(p64.float().to(dev)), p64.sum(1), "exact K13 outer")
    assert_exact_range({"bf16 result": p64[0].sum(0)})
    gb = ops._sum_partials(p64[0].float().to(dev), BF16)
    assert gb.dtype == BF16
    assert_exact(gb, p64[0].sum(0), "exact K13 bf16 out")
    for M, N, ld, dtype in ((1, 4, 4, F32), (127, 40, 40, BF16), (129, 260, 264, F32), (1000, 1024, 1024, BF16),
                            (300, 16, 4112, BF16)):
        b64 = ternary((M, ld), DENSITY, g, F64)
        x = b64.to(dtype).to(dev)[:, :N]
        ref = b64[:, :N].sum(0)
        assert_exact_range({"column sums": ref}, limit=F32_LIMIT)
        got = ops.column_sum(x)
        assert got.dtype == F32 and got.shape == (N,)
        assert_exact(got, ref, f"exact K13a {M}x{N} {dtype}")
    for n in (4096, 1028, 7):
        v64 = ternary((n,), DENSITY, g, F64)
        assert_exact(ops._sum_vector(v64.float().to(dev)), v64.sum(), f"exact vector sum n={n}")


# ----------------------------------------------------------------------------- short convolution
def check_exact_conv(dev, B, T, D, W, dtype, use_bias=False, seed=13):
    """K3 / K3b with ``activation=None``: y, dx, dw, dbias on ternary x, w, bias, dy and a 0/1 mask, against fp64 autograd
    through the oracle convolution."""
    g = torch.Generator().manual_seed(8000 + seed)
    x64, w64 = ternary((B, T, D), DENSITY, g, F64), ternary((D, 1, W), DENSITY, g, F64)
    b64 = ternary((D,), DENSITY, g, F64) if use_bias else None
    mask = (torch.rand(B, T, generator=g) > 0.2).to(F64)
    dy64 = ternary((B, T, D), DENSITY, g, F64)
    rl = [None if t is None else t.clone().requires_grad_(True) for t in (x64, w64, b64)]
    ry = O.short_conv(rl[0], rl[1], mask, None, activation=None, bias=rl[2])
    (ry * dy64).sum().backward()
    rng = {"x": x64, "w": w64, "bias": b64, "dy": dy64, "y": ry.detach(), "dx": rl[0].grad, "dw": rl[1].grad,
           "dbias": None if b64 is None else rl[2].grad}
    assert_exact_range(rng)
    ml = [None if t is None else t.to(dtype).to(dev).requires_grad_(True) for t in (x64, w64, b64)]
    y = ops.short_conv(ml[0], ml[1], ml[2], mask.float().to(dev), None, None)
    tag = f"exact short_conv B{B} T{T} D{D} W{W} {dtype} bias={use_bias}"
    assert_exact(y, ry.detach(), f"{tag}: y")
    (y.float() * dy64.to(dtype).to(dev).float()).sum().backward()
    assert_exact(ml[0].grad, rl[0].grad, f"{tag}: dx")
    assert ml[1].grad.shape == ml[1].shape
    assert_exact(ml[1].grad, rl[1].grad, f"{tag}: dw")
    if use_bias:
        assert_exact(ml[2].grad, rl[2].grad, f"{tag}: dbias")
    y0 = ops.short_conv(ml[0].detach(), ml[1].detach(), None if ml[2] is None else ml[2].detach(), mask.float().to(dev),
                        None, None)
    assert_exact(y0, ry.detach(), f"{tag}: y (no grad)")


# ----------------------------------------------------------------------------- the training GEMM path
def _train_refs(x64, w64, b64, dy64):
    n_in, n_out = x64.shape[-1], w64.shape[0]
    x2, dy2 = x64.reshape(-1, n_in), dy64.reshape(-1, n_out)
    y = x64 @ w64.t() + (0 if b64 is None else b64)
    dx = (dy2 @ w64).view(x64.shape)
    dw = dy2.t() @ x2
    db = dy2.sum(0)
    assert_exact_range({"x": x64, "W": w64, "b": b64, "dy": dy64, "y": y, "dx": dx})
    assert_exact_range({"dW": dw, "db": db}, limit=F32_LIMIT)
    return y, dx, dw, db


def check_exact_linear_train(dev, n_out, n_in, bias, autocast=True, B=3, T=100, seed=14):
    """``ops.linear`` under bf16 autocast with fp32 master weights (ternary x, W, b, dy): y (bf16), dx, dW, db (fp32) exact;
    and ``ops.linear_weight_grad`` forced to the token-split batched form (split = 4) on the same operands."""
    g = torch.Generator().manual_seed(9000 + seed)
    x64, w64 = ternary((B, T, n_in), DENSITY, g, F64), ternary((n_out, n_in), DENSITY, g, F64)
    b64 = ternary((n_out,), DENSITY, g, F64) if bias else None
    dy64 = ternary((B, T, n_out), DENSITY, g, F64)
    ry, rdx, rdw, rdb = _train_refs(x64, w64, b64, dy64)
    x, w = x64.float().to(dev).requires_grad_(), w64.float().to(dev).requires_grad_()
    b = None if b64 is None else b64.float().to(dev).requires_grad_()
    if autocast:
        with torch.autocast("cuda", dtype=BF16):
            y = ops.linear(x, w, b)
        assert y.dtype == BF16
    else:
        y = ops.linear(x, w, b)
    assert type(y.grad_fn).__name__ == "_LinearFunctionBackward", type(y.grad_fn).__name__
    tag = f"exact train linear {n_out}x{n_in} bias={bias} autocast={autocast}"
    assert_exact(y, ry, f"{tag}: y")
    (y.float() * dy64.float().to(dev)).sum().backward()
    assert x.grad.dtype == F32 and w.grad.dtype == F32
    assert_exact(x.grad, rdx, f"{tag}: dx")
    assert_exact(w.grad, rdw, f"{tag}: dW")
    if bias:
        assert_exact(b.grad, rdb, f"{tag}: db")
    cd = BF16 if autocast else F32
    assert (B * T) % 4 == 0
    dw4 = ops.linear_weight_grad(dy64.to(cd).to(dev).view(-1, n_out), x64.to(cd).to(dev).view(-1, n_in), split=4)
    assert dw4.dtype == F32
    assert_exact(dw4, rdw, f"{tag}: dW, token-split in four")


def check_exact_stacked_linear(dev, rows, n_in, pad, B, T, autocast, expect_split, expect_token_split=None, seed=15):
    """``ops.stacked_linear`` (K16 stacked operand; the 256-aligned main + narrow tail form of the GEMMs when
    ``expect_split``; the token-split dW of the main rows when ``expect_token_split``): y with exactly-zero pad columns, dx
    and every block's dW exact."""
    g = torch.Generator().manual_seed(9500 + seed)
    parts64 = [ternary((r, n_in), DENSITY, g, F64) for r in rows]
    x64 = ternary((B, T, n_in), DENSITY, g, F64)
    n_out = sum(rows) + pad
    dy64 = ternary((B, T, n_out), DENSITY, g, F64)
    w64 = torch.cat(parts64 + [torch.zeros(pad, n_in, dtype=F64)], 0)
    ry, rdx, rdw, _ = _train_refs(x64, w64, None, dy64)
    parts = [p.float().to(dev).requires_grad_() for p in parts64]
    x = x64.float().to(dev).requires_grad_()
    if autocast:
        with torch.autocast("cuda", dtype=BF16):
            y = ops.stacked_linear(x, parts, pad)
        assert y.dtype == BF16
    else:
        y = ops.stacked_linear(x, parts, pad)
    assert type(y.grad_fn).__name__ == "_StackedLinearFunctionBackward", type(y.grad_fn).__name__
    main = y.grad_fn.main
    assert (main < n_out) == expect_split, main
    if expect_token_split is not None:          # the rule of _StackedLinearFunction.backward for the main rows
        M = B * T
        S = ops._linear_split(M, main, n_in)
        assert (main < n_out and (S > 1 or (M % 4 == 0 and M // 4 >= 2048))) == expect_token_split
    tag = f"exact stacked linear rows={rows} n_in={n_in} tokens={B * T} autocast={autocast}"
    assert_exact(y, ry, f"{tag}: y")
    (y.float() * dy64.float().to(dev)).sum().backward()
    assert_exact(x.grad, rdx, f"{tag}: dx")
    r0 = 0
    for i, (p, r) in enumerate(zip(parts, rows)):
        assert p.grad.dtype == F32 and p.grad.is_contiguous()
        assert_exact(p.grad, rdw[r0:r0 + r], f"{tag}: dW[{i}]")
        r0 += r
