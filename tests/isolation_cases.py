"""The table of ops held to the row-isolation checks of ``tests/isolation.py``: one ``Op`` per kernel family, form and shape.

Shapes follow the smallest tail shapes of ``test_guard_bands.py`` / ``test_exact_gpu.py`` for the same family; row counts cross
a 16-row tile and the main / tail split (5, 17, 40), tall forms run at 130 rows with the tiling forced.  ``table(gpu=False)``
is the list the emulator runs (narrower widths where a case would take it more than a few seconds), ``table(gpu=True)`` the
device's full table.

Every factory returns an ``isolation.Op``; ``dev`` is "cpu" (ops bound to the wave64 emulator) or "cuda".  Inputs are i.i.d.
and DIFFERENT in every unit, so a unit that picked up a neighbour's data cannot hide behind equal values.
"""
import contextlib
import os

import pytest
import torch
import torch.nn.functional as F

import isolation as I
from isolation import Flat, Op
from kernel_cases import LibCalls
from lina_speech_amd import ops

BF16, F32 = torch.bfloat16, torch.float32


# ----------------------------------------------------------------------------- helpers
@contextlib.contextmanager
def _env(**kv):
    """Set (value None: unset) environment variables the launchers read at every call; restored on exit."""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _kq(dtype):
    return 32 if dtype == BF16 else 16


def _name(dtype):
    return "bf16" if dtype == BF16 else "f32"


def _nan_like(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _kernel_run(run, *symbols):
    """``run`` with the assertion that it reached every C entry point of ``symbols`` (the differentiable ops fall back to
    torch for shapes they are not built for: a case that silently took the fall-back would check torch, not the kernel)."""
    def checked(i):
        with LibCalls() as calls:
            out = run(i)
        for s in symbols:
            assert calls.of(s), f"{s} was not launched: {sorted({n for n, _ in calls.calls})}"
        return out
    return checked


# ----------------------------------------------------------------------------- projections
def op_linear(M, N, K, dtype, ln=False, bias=False, resid=False, swiglu=0, form="rows", variant=None):
    """``linear_skinny`` (``form`` "rows": row-major operands, with a fragment-major output copy), ``linear_skinny_packed``
    ("packed": fragment-major a and w built from the rows it is given) and the tall tiling ("tall": LINA_TALL = 1 forced, LINA_TALL_V =
    ``variant``, so the smaller launches of the subset check keep the kernel).  Unit: a row of ``a`` (and of the residual).
    Outputs: the row-major result, the fragment-major copy (through unpack_rows), and with a residual the in-place form
    (row-major: out = resid; packed: the residual stream held fragment-major only)."""
    n_w = 2 * swiglu if swiglu else N
    Np = (N + _kq(dtype) - 1) // _kq(dtype) * _kq(dtype)
    half = (N + 63) // 64 * 64 if swiglu else None
    kw = dict(swiglu_hidden=swiglu, ln_dim=K if ln else 0)

    def make(dev):
        g = _gen(9 + M + N)
        a = (torch.randn(M, K, generator=g) * 1.5 + (0.7 if ln else 0.0)).to(dtype).to(dev)
        w = (torch.randn(n_w, K, generator=g) / K ** 0.5).to(dtype).to(dev)
        c1 = w.float().sum(1).contiguous() if ln else None
        c2 = torch.randn(n_w, generator=g).to(dev) if (bias or ln) else None
        r = torch.randn(M, N, generator=g).to(dtype).to(dev) if resid else None
        return dict(a=a, w=w, c1=c1, c2=c2, r=r)

    def run(i):
        a, w, c1, c2, r = i["a"], i["w"], i["c1"], i["c2"], i["r"]
        m, dev = a.shape[0], a.device
        res = dict(inplace=None)
        out_p = torch.zeros(ops.packed_numel(m, Np), dtype=dtype, device=dev)
        if form == "rows":
            res["out"] = ops.linear_skinny(a, w, c1, c2, resid=r, n_out=N, out_packed=out_p, out_packed_width=Np, **kw)
            if r is not None:
                r2 = r.clone()
                ops.linear_skinny(a, w, c1, c2, resid=r2, out=r2, n_out=N, **kw)
                res["inplace"] = r2
        else:
            a_p = ops.pack_rows(a)
            if swiglu:
                pad = lambda h: torch.cat([h, torch.zeros(half - h.shape[0], K, dtype=dtype, device=dev)])
                w_p = torch.cat([ops.pack_rows(pad(w[:swiglu])), ops.pack_rows(pad(w[swiglu:]))])
            else:
                w_p = ops.pack_rows(w)
            env = dict(LINA_TALL="1", LINA_TALL_V=variant) if form == "tall" else dict(LINA_TALL="0")
            with _env(**env):
                out = _nan_like((m, N), dtype, dev)
                ops.linear_skinny_packed(a_p, w_p, m, N, K, c1, c2, resid=r, out=out, out_packed=out_p, out_packed_width=Np,
                                         w_half_rows=half, **kw)
                res["out"] = out
                if r is not None:
                    rp = torch.zeros(m, Np, dtype=dtype, device=dev)
                    rp[:, :N] = r
                    x_p = ops.pack_rows(rp)
                    ops.linear_skinny_packed(a_p, w_p, m, N, K, c1, c2, resid=x_p, out_packed=x_p, out_packed_width=Np,
                                             w_half_rows=half, **kw)
                    res["inplace"] = ops.unpack_rows(x_p, m, Np)
        res["out_packed"] = ops.unpack_rows(out_p, m, Np)
        return res

    tag = f"linear-{form}{'' if variant is None else f'-v{variant}'}-M{M}-N{N}-K{K}-{_name(dtype)}" \
          f"{'-ln' if ln else ''}{'-bias' if bias else ''}{'-resid' if resid else ''}{f'-swiglu{swiglu}' if swiglu else ''}"
    return Op(tag, make, run, (M,), dict(a=0, r=0, w=None, c1=None, c2=None), dict(out=0, out_packed=0, inplace=0))


def op_inproj(B, K, Kd, Vd, dtype, form="rows", variant=None):
    """The fused input side of a mixer over TWO consecutive steps (the second reads the conv caches the first rolled):
    ``gla_decode_inproj`` ("rows"), ``gla_decode_inproj_packed`` ("packed"), its tall tiling ("tall", forced, LINA_TALL_V =
    ``variant``) and ``gla_decode_prologue`` ("prologue": the projection row z is the input).  Unit: a row of x with its
    three conv caches."""
    R, W = 16, 4
    n_w = 2 * Kd + 2 * Vd + R

    def make(dev):
        g = _gen(23 + B)
        mk = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(dtype).to(dev)
        wide = n_w + 5 if form == "prologue" else K
        x = (torch.randn(2, B, wide, generator=g) + 0.3).to(dtype).to(dev)
        w_in = (torch.randn(n_w, K, generator=g) / K ** 0.5).to(dtype).to(dev)
        return dict(x=x, w_in=w_in, c1=w_in.float().sum(1).contiguous(), c2=torch.randn(n_w, generator=g).to(dev),
                    wq=mk(Kd, W), wk=mk(Kd, W), wv=mk(Vd, W), w2=mk(Kd, R), b2=mk(Kd), cq=mk(B, Kd, W), ck=mk(B, Kd, W),
                    cv=mk(B, Vd, W))

    def run(i):
        x, dev = i["x"], i["x"].device
        b = x.shape[1]
        cq, ck, cv = i["cq"], i["ck"], i["cv"]
        clamp = -0.03 if Kd == 128 else None
        res = {}
        env = dict(LINA_TALL="1", LINA_TALL_V=variant) if form == "tall" else dict(LINA_TALL="0")
        with _env(**env):
            w_p = ops.pack_rows(i["w_in"]) if form in ("packed", "tall") else None
            for s in range(2):
                qkv = _nan_like((b, 2 * Kd + Vd), dtype, dev)
                go = _nan_like((b, Vd), dtype, dev)
                gk = _nan_like((b, Kd), F32, dev)
                xs = x[s].contiguous()
                tail = (i["wq"], i["wk"], i["wv"], cq, ck, cv, i["w2"], i["b2"], qkv)
                if form == "prologue":
                    ops.gla_decode_prologue(xs, 0, Kd, 2 * Kd, 2 * Kd + 2 * Vd, *tail, gk, 16.0, clamp)
                    go = None
                elif form == "rows":
                    ops.gla_decode_inproj(xs, i["w_in"], i["c1"], i["c2"], *tail, go, gk, clamp_min=clamp)
                else:
                    ops.gla_decode_inproj_packed(ops.pack_rows(xs), w_p, b, K, i["c1"], i["c2"], *tail, go, gk, clamp_min=clamp)
                res.update({f"qkv{s}": qkv, f"g{s}": go, f"gk{s}": gk})
        res.update(cq=cq, ck=ck, cv=cv)
        return res

    shared = dict(w_in=None, c1=None, c2=None, wq=None, wk=None, wv=None, w2=None, b2=None)
    outs = dict(qkv0=0, g0=0, gk0=0, qkv1=0, g1=0, gk1=0, cq=0, ck=0, cv=0)
    tag = f"inproj-{form}{'' if variant is None else f'-v{variant}'}-B{B}-K{K}-{Kd}x{Vd}-{_name(dtype)}"
    return Op(tag, make, run, (B,), dict(x=1, cq=0, ck=0, cv=0, **shared), outs)


def op_swiglu(M, hidden, dtype):
    """``ops.swiglu`` (the decode step's gate; plain and padded with the constant-1 column).  Unit: a row."""
    def make(dev):
        return dict(u=torch.randn(M, 2 * hidden, generator=_gen(6)).to(dtype).to(dev))

    def run(i):
        return dict(y=ops.swiglu(i["u"], hidden), y_pad=ops.swiglu(i["u"], hidden, pad_to=hidden + 3))

    return Op(f"swiglu-M{M}-{hidden}-{_name(dtype)}", make, run, (M,), dict(u=0), dict(y=0, y_pad=0))


# ----------------------------------------------------------------------------- K1d, K1d + K5, K5 over partial sums
def op_decode_update(B, H, Dk, Dv, dtype, fused):
    """K1d ``gla_decode_update`` (``fused`` False) / K1d + K5 ``gla_decode_update_norm`` over two steps on the same state.
    Unit: (b, h) with its state.  Dk = 256: four row-block workgroups per head; in the fused form the last to arrive sums the
    partials of ITS head and norms them -- a neighbour's ``o_part`` slice picked up there would show.  The arrival counters
    are an output: left at zero for every head."""
    NP = Dk // 64

    def make(dev):
        g = _gen(13 + B * H)
        mk = lambda *s: torch.randn(*s, generator=g).to(dtype).to(dev)
        gk = (F.logsigmoid(torch.randn(2, B, H, Dk, generator=g) * 2.0) / 4.0).to(dev)
        return dict(q=mk(2, B, H, Dk), k=mk(2, B, H, Dk), v=mk(2, B, H, Dv), gk=gk, gate=mk(2, B, H, Dv),
                    S=(torch.randn(B, H, Dk, Dv, generator=g) * 0.5).to(dev),
                    w=(1 + 0.1 * torch.randn(Dv, generator=g)).to(dtype).to(dev))

    def run(i):
        S, dev = i["S"], i["S"].device
        b, h = S.shape[:2]
        counters = torch.zeros(b * h, dtype=torch.int32, device=dev)
        res = dict(S=S, counters=counters)
        for s in range(2):
            o_part = _nan_like((NP, b, h, Dv), F32, dev)
            q, k, v, gk, gate = (i[n][s].contiguous() for n in ("q", "k", "v", "gk", "gate"))
            if fused:
                og = _nan_like((b, h, Dv), dtype, dev)
                ops.gla_decode_update_norm(q, k, v, gk, o_part, S, gate, i["w"], og, counters, 1e-5)
            else:
                ops.gla_decode_update(q, k, v, gk, o_part, S)
                og = ops.rmsnorm_swish_gate(o_part, gate, i["w"], 1e-5, n_partial=NP, out_dtype=dtype).reshape(b, h, Dv)
            res.update({f"o_part{s}": o_part, f"og{s}": og})
        return res

    tag = f"{'k1d+k5' if fused else 'k1d,k5-partials'}-B{B}-H{H}-{Dk}x{Dv}-{_name(dtype)}"
    return Op(tag, make, run, (B, H), dict(q=1, k=1, v=1, gk=1, gate=1, S=0, w=None),
              dict(S=0, counters=Flat(0), o_part0=1, og0=0, o_part1=1, og1=0))


# ----------------------------------------------------------------------------- K1w
def op_decode_window(B, H, Dk, Dv, dtype, state_dtype=F32, window=8, n_wg=0, packed=False):
    """K1w ``gla_decode_window`` over window + 1 steps (a completed window writes the state back; one more step opens the
    next window) and ``gla_decode_window_flush`` of the pending step.  ``n_wg`` > 0: the persistent form (kept in the smaller
    launches of the subset check: more workgroups than heads is a served grid).  Dv = 512: the column halves of a head meet
    in ``o_exchange``.  ``packed``: og written fragment-major ([B, H * Dv] rows), read back through unpack_rows.  Unit: (b, h)
    with its state; the history buffers start as NaN everywhere (a stale entry of ANY slot that is read shows) and are
    outputs; a gate reset (-20) sits inside the window."""
    n_steps = window + 1

    def make(dev):
        g = _gen(14 + B * H + window)
        mk = lambda *s: torch.randn(*s, generator=g).to(dtype).to(dev)
        gk = F.logsigmoid(torch.randn(n_steps, B, H, Dk, generator=g) * 2.0) / 4.0
        gk[min(3, n_steps - 1), :, :, ::2] = -20.0
        return dict(q=mk(n_steps, B, H, Dk), k=mk(n_steps, B, H, Dk), v=mk(n_steps, B, H, Dv), gk=gk.to(dev),
                    gate=mk(n_steps, B, H, Dv), S=(torch.randn(B, H, Dk, Dv, generator=g) * 0.5).to(state_dtype).to(dev),
                    w=(1 + 0.1 * torch.randn(Dv, generator=g)).to(dtype).to(dev))

    def run(i):
        S, dev = i["S"], i["S"].device
        b, h = S.shape[:2]
        hk, hc = (_nan_like((window, b * h, Dk), F32, dev) for _ in range(2))
        hv = _nan_like((window, b * h, Dv), F32, dev)
        counters = torch.zeros(b * h, dtype=torch.int32, device=dev)
        o_x = _nan_like((b * h * Dv,), F32, dev) if Dv > 256 else None
        origin = torch.full((1,), 5, dtype=torch.int64, device=dev)
        ogs, S_window = [], None
        for t in range(n_steps):
            step = torch.full((1,), 5 + t, dtype=torch.int64, device=dev)
            q, k, v, gk, gate = (i[n][t].contiguous() for n in ("q", "k", "v", "gk", "gate"))
            if packed:
                og = _nan_like((ops.packed_numel(b, h * Dv),), dtype, dev)
            else:
                og = _nan_like((b, h, Dv), dtype, dev)
            ops.gla_decode_window(q, k, v, gk, S, gate, i["w"], og, hk, hc, hv, step, origin, window, 1e-5, og_packed=packed,
                                  o_exchange=o_x, counters=counters, n_wg=n_wg)
            ogs.append(ops.unpack_rows(og, b, h * Dv).view(b, h, Dv) if packed else og)
            if t == window - 1:
                S_window = S.clone()
        hist = dict(hk=hk.clone(), hc=hc.clone(), hv=hv.clone())
        ops.gla_decode_window_flush(S, hk, hc, hv, n_steps % window)
        return dict(og=torch.stack(ogs), S_window=S_window, S=S, counters=counters, **hist)

    tag = f"k1w-B{B}-H{H}-{Dk}x{Dv}-{_name(dtype)}-state-{_name(state_dtype)}-window{window}-nwg{n_wg}{'-packed' if packed else ''}"
    return Op(tag, make, run, (B, H), dict(q=1, k=1, v=1, gk=1, gate=1, S=0, w=None),
              dict(og=1, S_window=0, S=0, counters=Flat(0), hk=Flat(1), hc=Flat(1), hv=Flat(1)))


# ----------------------------------------------------------------------------- cross-attention
CROSS_PARTS = ("scores", "spe", "add", "steps", "pe")


def op_cross(B, Tn, d, dtype, parts=CROSS_PARTS):
    """The uniform cross-attention launches, each on its own buffers, in groups (``parts``): "scores" = ``cross_scores``,
    ``softmax_rows``, ``cross_scores_softmax``; "spe" = ``softmax_pe_rows`` with the fragment-major copy of xp and the att-log
    form; "add" = ``weighted_rows_add`` and ``softmax_weighted_rows_add`` (row-major and packed x); "steps" =
    ``cross_att_step1`` / ``step2``; "pe" (d % 256 == 0 only) = ``pe_softmax_weighted_rows_add`` (row-major, packed xp and x,
    att-log form).  Unit: a batch row with its kk and vv rows; the positional table and the LayerNorm parameters are shared.
    "spe", "add" and "pe" write fragment-major rows (16-row tiles); the others run one workgroup per row."""
    Tp = (Tn + 31) // 32 * 32
    scale = d ** -0.5
    pk = d % _kq(dtype) == 0
    parts = tuple(p for p in parts if p != "pe" or d % 256 == 0)
    cap = 4

    def make(dev):
        g = _gen(15 + B + Tn)
        mk = lambda *s: torch.randn(*s, generator=g).to(dtype).to(dev)
        return dict(q_lin=mk(B, d), kk=mk(B, Tn, d), vv=mk(B, Tn, d), x=mk(B, d), xp=mk(B, d), sc=mk(B, Tp) * 3,
                    sc32=(torch.randn(B, Tn, generator=g) * 2).to(dev), attc=torch.softmax(mk(B, Tp).float(), -1).to(dtype),
                    pe=mk(Tp + 3, d), ln_w=(1 + 0.1 * torch.randn(d, generator=g)).to(dtype).to(dev),
                    ln_b=(0.1 * torch.randn(d, generator=g)).to(dtype).to(dev))

    def run(i):
        q_lin, kk, vv, x0, xp0, pe, ln_w, ln_b = (i[n] for n in ("q_lin", "kk", "vv", "x", "xp", "pe", "ln_w", "ln_b"))
        b, dev = q_lin.shape[0], q_lin.device
        att = lambda: torch.zeros(b, 2, 1, Tn, dtype=dtype, device=dev)
        attc = lambda: _nan_like((b, Tp), dtype, dev)
        step = torch.full((1,), 2, dtype=torch.int64, device=dev)
        res = {}
        if "scores" in parts:
            scores = _nan_like((b, Tn), F32, dev)
            ops.cross_scores(q_lin, ln_w, ln_b, 1e-5, kk, scores, scale)
            a1, c1 = att(), attc()
            ops.softmax_rows(scores, 1.0, a1[:, 1, 0], c1, Tn)
            a3, c3 = att(), attc()
            ops.cross_scores_softmax(q_lin, ln_w, ln_b, 1e-5, kk, a3[:, 0, 0], c3, scale)
            res.update(scores=scores, softmax_att=a1, softmax_attc=c1, css_att=a3, css_attc=c3)
        if "spe" in parts:
            a2, xp = att(), _nan_like((b, d), dtype, dev)
            xp_p = torch.zeros(ops.packed_numel(b, d), dtype=dtype, device=dev) if pk else None
            ops.softmax_pe_rows(i["sc32"], a2[:, 0, 0], pe, xp, xp_p)
            log = torch.full((b, 2, cap, Tn), 7.0, dtype=dtype, device=dev)
            xp2 = _nan_like((b, d), dtype, dev)
            ops.softmax_pe_rows(i["sc32"], log[:, 0, 0], pe, xp2, None, att_step=step, att_step_stride=log.stride(2), att_steps=cap)
            res.update(spe_att=a2, spe_xp=xp, spe_xp_packed=ops.unpack_rows(xp_p, b, d) if pk else None, spe_log=log, spe_log_xp=xp2)
        if "add" in parts:
            c1 = i["attc"].clone()
            c1[:, Tn:] = 0
            x1 = x0.clone()
            ops.weighted_rows_add(c1, vv, x1)
            x1p = ops.pack_rows(x0) if pk else None
            if pk:
                ops.weighted_rows_add(c1, vv, x0.clone(), x_packed=x1p)
            a4, x2 = att(), x0.clone()
            ops.softmax_weighted_rows_add(i["sc"], scale, a4[:, 1, 0], vv, x2)
            x2p = ops.pack_rows(x0) if pk else None
            if pk:
                ops.softmax_weighted_rows_add(i["sc"], scale, att()[:, 1, 0], vv, x0.clone(), x_packed=x2p)
            res.update(wra_x=x1, wra_x_packed=ops.unpack_rows(x1p, b, d) if pk else None, swra_att=a4, swra_x=x2,
                       swra_x_packed=ops.unpack_rows(x2p, b, d) if pk else None)
        if "steps" in parts:
            a5, xp5 = att(), _nan_like((b, d), dtype, dev)
            ops.cross_att_step1(q_lin, ln_w, ln_b, 1e-5, kk, pe, a5[:, 0, 0], xp5, scale)
            x5 = x0.clone()
            ops.cross_att_step2(xp0, pe, vv, a5[:, 1, 0], x5, scale)
            res.update(step_att=a5, step1_xp=xp5, step2_x=x5)
        if "pe" in parts:
            a6, x6 = att(), x0.clone()
            ops.pe_softmax_weighted_rows_add(xp0, pe, scale, a6[:, 1, 0], vv, x6)
            x6p = ops.pack_rows(x0)
            ops.pe_softmax_weighted_rows_add(ops.pack_rows(xp0), pe, scale, att()[:, 1, 0], vv, x0.clone(), x_packed=x6p,
                                             xp_is_packed=True)
            log6, x7 = torch.full((b, 2, cap, Tn), 7.0, dtype=dtype, device=dev), x0.clone()
            ops.pe_softmax_weighted_rows_add(xp0, pe, scale, log6[:, 1, 0], vv, x7, att_step=step,
                                             att_step_stride=log6.stride(2), att_steps=cap)
            res.update(pe_att=a6, pe_x=x6, pe_x_packed=ops.unpack_rows(x6p, b, d), pe_log=log6, pe_log_x=x7)
        return res

    outs = dict(scores=("scores", "softmax_att", "softmax_attc", "css_att", "css_attc"),
                spe=("spe_att", "spe_xp", "spe_xp_packed", "spe_log", "spe_log_xp"),
                add=("wra_x", "wra_x_packed", "swra_att", "swra_x", "swra_x_packed"), steps=("step_att", "step1_xp", "step2_x"),
                pe=("pe_att", "pe_x", "pe_x_packed", "pe_log", "pe_log_x"))
    tag = f"cross-B{B}-Tn{Tn}-d{d}-{_name(dtype)}{'' if len(parts) >= 4 else '-' + '+'.join(parts)}"
    return Op(tag, make, run, (B,),
              dict(q_lin=0, kk=0, vv=0, x=0, xp=0, sc=0, sc32=0, attc=0, pe=None, ln_w=None, ln_b=None),
              {n: 0 for p in parts for n in outs[p]})


# ----------------------------------------------------------------------------- picks, sampling, embedding
def op_argmax(M, n, dtype):
    def make(dev):
        lg = torch.randn(M, n, generator=_gen(5)).to(dtype)
        lg[1, 3] = lg[1, n - 2] = 50.0            # an exact tie: the lowest index
        lg[2, n - 1] = 60.0
        return dict(logits=lg.to(dev))

    return Op(f"argmax-M{M}-n{n}-{_name(dtype)}", make, lambda i: dict(tok=ops.argmax_rows(i["logits"])), (M,), dict(logits=0),
              dict(tok=0), index_outputs=dict(tok=(0, n)))


def op_topk(M, n, k, dtype, hashed=False):
    """K6c ``topk_sample_rows``.  Supplied uniforms ``u`` (a unit input: poisoned with the row): all checks.  ``hashed``: the
    uniform of a row is hash(seed, step, ROW INDEX), so a row moved to another slot or launched in a smaller batch
    legitimately draws another number -- only the poisoned-neighbours check and the in-place subset check (same slot, same
    row count, every other row overwritten) apply."""
    def make(dev):
        g = _gen(3 + M)
        d = dict(logits=(torch.randn(M, n, generator=g) * 3).to(dtype).to(dev))
        if not hashed:
            d["u"] = torch.rand(M, generator=g).to(dev)
        return d

    def run(i):
        if hashed:
            step = torch.full((1,), 5, dtype=torch.int64, device=i["logits"].device)
            return dict(tok=ops.topk_sample_rows(i["logits"], k, 0.8, seed=1234, step=step))
        return dict(tok=ops.topk_sample_rows(i["logits"], k, 0.8, u=i["u"]))

    ins = dict(logits=0) if hashed else dict(logits=0, u=0)
    return Op(f"topk-{'hashed' if hashed else 'u'}-M{M}-n{n}-k{k}-{_name(dtype)}", make, run, (M,), ins, dict(tok=0),
              index_outputs=dict(tok=(0, n)), checks=("poisoned", "subset_in_place") if hashed else Op.checks)


def op_embed_sum(Q, B, n, n_emb, d, dtype):
    def make(dev):
        g = _gen(4)
        return dict(table=torch.randn(Q, n_emb, d, generator=g).to(dtype).to(dev),
                    idx=torch.randint(0, n_emb, (Q, B, n), generator=g).to(dev))

    alt = lambda i: dict(idx=(i["idx"] + 1 + i["idx"] % 5) % n_emb)
    return Op(f"embed-sum-Q{Q}-B{B}-{_name(dtype)}", make, lambda i: dict(out=ops.embed_sum(i["table"], i["idx"])), (B,),
              dict(table=None, idx=1), dict(out=0), alt_ints=alt)


def op_pick(B, Q, L, d, dtype, mode, n_sampled=0, steps=4):
    """K6d ``greedy_pick_embed`` / K6e ``sample_pick_embed`` / K6f ``pick_embed_forced`` over ``steps`` steps with a loop-control
    block: the ``tok_log`` columns, the next-input rows (row-major and fragment-major) and the per-row words of the control
    block belong to the row.  SHARED outputs, excluded: the header of the control block (word 0 counts the stopped rows of
    the whole batch, word 1 is the first step at which ALL rows have stopped, words 2-3 the seed) and the step counter.
    Some rows pick the stop token on every quantizer at some step (their flag is set), one row on one quantizer only (it is
    not).  Sampled quantizers (``n_sampled`` > 0) draw hash(seed, step, b * Q + q): row-index dependent, so only the
    poisoned-neighbours and the in-place subset check apply (see ``op_topk``)."""
    n_emb = L + 3
    R = ops.LOOP_CTL_ROWS
    P = steps - 1

    def make(dev):
        g = _gen(17 + B + Q)
        logits = torch.randn(steps, B, Q, L, generator=g)
        logits[:, :, :, 2] = -40.0
        for t in range(steps):
            for b_ in range(B):
                if (b_ + t) % 5 == 1:
                    logits[t, b_, :, 2] = 40.0                     # row b stops at step t
                elif (b_ + t) % 5 == 3:
                    logits[t, b_, 0, 2] = 40.0                     # one quantizer only: not a stop
        logits[0, 0, 0, 5] = logits[0, 0, 0, 9] = 50.0             # an exact tie: the lowest index
        d_ = dict(logits=logits.to(dtype).to(dev), table=torch.randn(Q, n_emb, d, generator=g).to(dtype).to(dev))
        if mode == "forced":
            d_["force_tok"] = torch.randint(0, n_emb, (P, Q, B), generator=g).to(dev)
            d_["force_len"] = torch.tensor([(0, 2, 5, 1, 7)[b_ % 5] for b_ in range(B)], dtype=torch.int32).to(dev)
        return d_

    def run(i):
        logits, table = i["logits"], i["table"]
        b, dev = logits.shape[1], logits.device
        tok_log = torch.full((steps, Q, b), -1, dtype=torch.int64, device=dev)
        step = torch.zeros(1, dtype=torch.int64, device=dev)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        ctl = ops.new_loop_ctl(b, dev, 0x9E3779B97F4A7C15 if n_sampled else 0)
        pk = d % _kq(dtype) == 0
        xs, xps = [], []
        for t in range(steps):
            x = _nan_like((b, d), dtype, dev)
            x_p = torch.zeros(ops.packed_numel(b, d), dtype=dtype, device=dev) if pk else None
            lg = logits[t].contiguous()
            if mode == "greedy":
                ops.greedy_pick_embed(lg, table, x, tok_log, step, counter, x_packed=x_p, loop_ctl=ctl)
            elif mode == "sample":
                ops.sample_pick_embed(lg, table, x, tok_log, step, counter, n_sampled, 7, 0.8, seed=11, x_packed=x_p, loop_ctl=ctl)
            else:
                ops.pick_embed_forced(lg, table, x, tok_log, step, counter, i["force_tok"], i["force_len"], n_sampled, 7, 0.8,
                                      seed=11, x_packed=x_p, loop_ctl=ctl)
            xs.append(x)
            xps.append(ops.unpack_rows(x_p, b, d) if pk else x)
        return dict(tok_log=tok_log, x=torch.stack(xs), x_packed=torch.stack(xps), ctl_rows=ctl[R:R + b].clone(),
                    ctl_head=ctl[:R].clone(), step=step, counter=counter)

    ins = dict(logits=1, table=None)
    alt = None
    if mode == "forced":
        ins.update(force_tok=2, force_len=0)
        alt = lambda i: dict(force_tok=(i["force_tok"] + 7) % n_emb, force_len=(i["force_len"] + 1) % (P + 2))
    return Op(f"pick-{mode}-B{B}-Q{Q}-L{L}-d{d}-{_name(dtype)}-sampled{n_sampled}", make, run, (B,), ins,
              dict(tok_log=2, x=1, x_packed=1, ctl_rows=0, ctl_head=None, step=None, counter=None), alt_ints=alt,
              index_outputs=dict(tok_log=(0, L)), checks=("poisoned", "subset_in_place") if n_sampled else Op.checks)


def check_rows_rearm(dev, B, d, dtype):
    """K6g ``rows_rearm`` re-arms the LISTED rows and nothing else.  (a) the unlisted rows poisoned (NaN, then +inf / 3e38, in
    their state rows and their x rows; set stop flags): the listed rows come out exactly as in the unpoisoned launch, and the
    unlisted rows keep their poison bit for bit.  (b) the listed rows poisoned beforehand: they come out clean -- state rows
    zero, x = the start embedding (row-major and fragment-major), stop flag cleared, the new text length -- and equal to
    (a)'s.  The header word 0 of the control block (the count of stopped rows of the whole batch) is shared and compared with
    its definition, not between launches."""
    g = _gen(71 + B)
    R = ops.LOOP_CTL_ROWS
    listed = torch.arange(B)[1::2][: max(1, B // 3)]
    if B > 17:
        listed = torch.cat([listed, torch.tensor([16, B - 1])]).unique()
    is_listed = torch.zeros(B, dtype=torch.bool)
    is_listed[listed] = True
    rows = listed.flip(0).to(torch.int32).to(dev)                       # any order
    new_len = (torch.arange(len(listed), dtype=torch.int32) + 3).to(dev)
    y_start = torch.randn(d, generator=g).to(dtype).to(dev)
    base = dict(conv=torch.randn(B, 24, 4, generator=g).to(dtype), state=torch.randn(B, 2, 16, 8, generator=g),
                state_bf=torch.randn(B, 2, 16, 8, generator=g).to(BF16), x=torch.randn(B, d, generator=g).to(dtype))
    flags0 = (torch.arange(B) % 3 != 0).to(torch.int32)
    pk = d % _kq(dtype) == 0

    def launch(poison, who):
        t = {n: v.clone() for n, v in base.items()}
        if poison is not None:
            for n, v in t.items():
                bad = I._poison_value(v, poison)
                t[n] = torch.where(who.view(-1, *[1] * (v.dim() - 1)), bad, v)
        t = {n: v.to(dev) for n, v in t.items()}
        x_p = ops.pack_rows(t["x"]) if pk else None
        ctl = ops.new_loop_ctl(B, dev)
        ctl[R:R + B] = flags0.to(dev)
        ctl[0] = int(flags0.sum())
        ctl[1] = 2
        txt_len = torch.full((B,), 9, dtype=torch.int32, device=dev)
        table = ops.RearmTable([t["conv"], t["state"], t["state_bf"]], B)
        ops.rows_rearm(rows, table, y_start, t["x"], x_packed=x_p, loop_ctl=ctl, txt_len=txt_len, new_len=new_len)
        out = dict(t, flags=ctl[R:R + B].clone(), txt_len=txt_len)
        if pk:
            out["x_packed"] = ops.unpack_rows(x_p, B, d)
        assert int(ctl[0]) == int(flags0[~is_listed].sum()) and int(ctl[1]) == -1, "control-block header after the re-arm"
        return out, t

    ref, _ = launch(None, None)
    L = listed.to(dev)
    for n in ("conv", "state", "state_bf"):
        assert float(ref[n][L].float().abs().max()) == 0.0, f"rows_rearm: {n} rows of the listed rows are not zero"
    assert torch.equal(ref["x"][L], y_start.expand(len(L), d)) and int(ref["flags"][L].abs().sum()) == 0
    assert torch.equal(ref["txt_len"][rows.long()], new_len)
    U = (~is_listed).nonzero().view(-1).to(dev)
    for n, v in base.items():
        assert torch.equal(I.bits(ref[n][U]), I.bits(v[U.cpu()])), f"rows_rearm: an unlisted row of {n} changed"
    assert torch.equal(ref["flags"][U].cpu(), flags0[~is_listed]) and bool((ref["txt_len"][U] == 9).all())
    for variant in ("nan", "inf"):
        for who, keep, what in ((~is_listed, L, "unlisted rows poisoned"), (is_listed, None, "listed rows poisoned")):
            got, _ = launch(variant, who)
            for n in ref:
                a, b_ = (got[n], ref[n]) if keep is None else (got[n][keep], ref[n][keep])
                assert torch.equal(I.bits(a), I.bits(b_)), f"rows_rearm ({what}, {variant}): {n} differs from the clean launch"
            if keep is not None:           # the unlisted rows keep their poison, bit for bit
                for n, v in base.items():
                    bad = I._poison_value(v, variant)[U.cpu()]
                    assert torch.equal(I.bits(got[n][U]), I.bits(bad)), f"rows_rearm ({what}, {variant}): unlisted {n} rows changed"


# ----------------------------------------------------------------------------- K1 / K2 / K2b
def _head_first(x):
    """[B,H,T,D] values laid out [B,T,H*D] in memory, seen head-first: how the projections hand them to the ops."""
    return x.transpose(1, 2).contiguous().transpose(1, 2)


def op_gla(fn, B, H, T, Dk, Dv, dtype, with_h0=True, nseg=None, dv512_one_launch=None, t0s=(45, 64), subset_units=None):
    """K1 ``fused_recurrent_gla`` / K2 ``chunk_gla`` (``nseg``: the segment-parallel form, forced) / ``fused_chunk_gla`` /
    ``chunk_simple_gla`` (a gate per head and token).  Unit: (b, h) with its initial state; outputs o and the final state.
    Time axis: o at positions < t0 does not change when q, k, v, g at positions >= t0 do (finite values: see isolation.py);
    the final state is not compared there.  ``dv512_one_launch``: the launch policy of 256 x 512 heads, set for the call.
    ``subset_units`` "rows": the kernel groups 2 or 4 heads per workgroup by H, so a head is not launched without its
    batch row's other heads."""
    simple = fn == "chunk_simple_gla"

    def make(dev):
        g = _gen(31 + B * H + T)
        mk = lambda D: torch.randn(B, H, T, D, generator=g).to(dtype).to(dev)
        if simple:
            gk = (F.logsigmoid(torch.randn(B, H, T, generator=g) * 2.0) / 4.0).to(dev)
        else:
            gk = (F.logsigmoid(torch.randn(B, H, T, Dk, generator=g) * 2.0) / 4.0)
            gk[:, :, min(17, T - 1), ::3] = -20.0  # a reset gate
            gk = gk.to(dtype).to(dev)
        return dict(q=mk(Dk), k=mk(Dk), v=mk(Dv), g=gk, h0=(torch.randn(B, H, Dk, Dv, generator=g) * 0.5).to(dev) if with_h0 else None)

    def run(i):
        q, k, v = (_head_first(i[n]) for n in ("q", "k", "v"))
        g = i["g"].contiguous() if simple else _head_first(i["g"])
        kw = dict(nseg=nseg) if fn == "chunk_gla" else {}
        prev = ops.POLICY.dv512_one_launch
        try:
            if dv512_one_launch is not None:
                ops.POLICY.dv512_one_launch = dv512_one_launch
            o, S = getattr(ops, fn)(q, k, v, g, initial_state=i["h0"], output_final_state=True, **kw)
        finally:
            ops.POLICY.dv512_one_launch = prev
        return dict(o=o.contiguous(), S=S)

    t0s = tuple(t for t in t0s if t < T)
    tag = f"{fn}-B{B}-H{H}-T{T}-{Dk}x{Dv}-{_name(dtype)}{'' if with_h0 else '-no-h0'}{'' if nseg is None else f'-nseg{nseg}'}" \
          f"{'' if dv512_one_launch is None else ('-one-launch' if dv512_one_launch else '-two-launches')}"
    return Op(tag, make, run, (B, H), dict(q=0, k=0, v=0, g=0, h0=0), dict(o=0, S=0),
              checks=("permutation", "poisoned", "subset", "time") if t0s else Op.checks,
              time_axes=dict(q=2, k=2, v=2, g=2, o=2), t0s=t0s, subset_units=subset_units)


def op_gla_bwd(B, H, T, Dk, Dv, dtype, path, nseg=None, subset_units=None):
    """K2b ``gla_chunk_bwd`` (``path`` "sweeps": the generic kernel, "full": the full-head sweeps on ``nseg`` segments): dq, dk,
    dv, dg, dh0 from d_o and the gradient of the final state.  Unit: (b, h); the final state handed to the backward is the
    forward's own (K1, computed once in ``make``)."""
    def make(dev):
        g = _gen(37 + B * H + T)
        mk = lambda D: torch.randn(B, H, T, D, generator=g).to(dtype).to(dev)
        gk = (F.logsigmoid(torch.randn(B, H, T, Dk, generator=g) * 2.0) / 4.0).to(dtype).to(dev)
        d = dict(q=mk(Dk), k=mk(Dk), v=mk(Dv), g=gk, d_o=mk(Dv), h0=(torch.randn(B, H, Dk, Dv, generator=g) * 0.5).to(dev),
                 d_ht=(torch.randn(B, H, Dk, Dv, generator=g) * 0.1).to(dev))
        _, d["ht"] = ops.fused_recurrent_gla(*(_head_first(d[n]) for n in ("q", "k", "v", "g")), initial_state=d["h0"],
                                             output_final_state=True)
        return d

    def run(i):
        q, k, v, g, d_o = (_head_first(i[n]) for n in ("q", "k", "v", "g", "d_o"))
        got = ops.gla_chunk_bwd(q, k, v, g, d_o, Dk ** -0.5, i["h0"], i["ht"], i["d_ht"], need_dh0=True, nseg=nseg, path=path)
        return {n: t.contiguous() for n, t in zip(("dq", "dk", "dv", "dg", "dh0"), got)}

    tag = f"k2b-{path}-B{B}-H{H}-T{T}-{Dk}x{Dv}-{_name(dtype)}{'' if nseg is None else f'-nseg{nseg}'}"
    return Op(tag, make, run, (B, H), dict(q=0, k=0, v=0, g=0, d_o=0, h0=0, ht=0, d_ht=0), dict(dq=0, dk=0, dv=0, dg=0, dh0=0),
              subset_units=subset_units)


# ----------------------------------------------------------------------------- row-wise training ops
def op_layer_norm(N, D, dtype, resid=True):
    """K10 ``layer_norm`` forward (y and, with a residual, x + r) and backward dx / dr.  Unit: a row.  The parameter
    gradients sum over all rows: shared outputs, not returned."""
    def make(dev):
        g = _gen(31 + N)
        mk = lambda: torch.randn(N, D, generator=g).to(dtype).to(dev)
        return dict(x=(torch.randn(N, D, generator=g) * 2 + 0.5).to(dtype).to(dev), r=mk() if resid else None, wy=mk(), ws=mk(),
                    gamma=(1 + 0.3 * torch.randn(D, generator=g)).to(dev), beta=(0.2 * torch.randn(D, generator=g)).to(dev))

    def run(i):
        x = i["x"].requires_grad_()
        r = None if i["r"] is None else i["r"].requires_grad_()
        gamma, beta = i["gamma"].requires_grad_(), i["beta"].requires_grad_()
        out = ops.layer_norm(x, gamma, beta, 1e-5, residual=r, out_dtype=dtype)
        y, xs = (out, None) if r is None else out
        loss = (y.float() * i["wy"].float()).sum() + ((xs.float() * i["ws"].float()).sum() if xs is not None else 0.0)
        loss.backward()
        return dict(y=y.detach(), xs=None if xs is None else xs.detach(), dx=x.grad, dr=None if r is None else r.grad)

    run = _kernel_run(run, "lina_layernorm_fwd", "lina_layernorm_bwd")
    return Op(f"layer-norm-N{N}-D{D}-{_name(dtype)}{'-resid' if resid else ''}", make, run, (N,),
              dict(x=0, r=0, wy=0, ws=0, gamma=None, beta=None), dict(y=0, xs=0, dx=0, dr=0))


def op_rmsnorm_bwd(N, D, dtype):
    """K5 / K5b ``rmsnorm_swish_gate`` forward and backward dx / dg (rows [N, 2, D]).  The weight gradient is shared."""
    def make(dev):
        g = _gen(13 + N)
        mk = lambda s=1.0: (torch.randn(N, 2, D, generator=g) * s).to(dtype).to(dev)
        return dict(x=mk(3), gate=mk(), dy=mk(), w=(1 + 0.1 * torch.randn(D, generator=g)).to(dtype).to(dev))

    def run(i):
        x, gate, w = i["x"].requires_grad_(), i["gate"].requires_grad_(), i["w"].requires_grad_()
        y = ops.rmsnorm_swish_gate(x, gate, w, 1e-5)
        (y.float() * i["dy"].float()).sum().backward()
        return dict(y=y.detach(), dx=x.grad, dgate=gate.grad)

    run = _kernel_run(run, "lina_rmsnorm_gate_fwd", "lina_rmsnorm_gate_bwd")
    return Op(f"rmsnorm-gate-bwd-N{N}-D{D}-{_name(dtype)}", make, run, (N,), dict(x=0, gate=0, dy=0, w=None), dict(y=0, dx=0, dgate=0))


def op_swiglu_gate(N, H, dtype):
    """K11 / K11b ``swiglu_gate`` and du (odd widths take the scalar kernels)."""
    def make(dev):
        g = _gen(37 + N)
        return dict(u=(torch.randn(N, 2 * H, generator=g) * 1.5).to(dtype).to(dev), w=torch.randn(N, H, generator=g).to(dtype).to(dev))

    def run(i):
        u = i["u"].requires_grad_()
        y = ops.swiglu_gate(u)
        (y.float() * i["w"].float()).sum().backward()
        return dict(y=y.detach(), du=u.grad)

    run = _kernel_run(run, "lina_swiglu", "lina_swiglu_bwd")
    return Op(f"swiglu-gate-N{N}-H{H}-{_name(dtype)}", make, run, (N,), dict(u=0, w=0), dict(y=0, du=0))


def op_gate(N, C, dtype, lowrank=0):
    """K12 ``gate_logsigmoid`` (and dx) / K12b ``gate_lowrank`` forward (``lowrank`` = L, the rank).  Unit: a row."""
    def make(dev):
        g = _gen(41 + N)
        if lowrank:
            return dict(x=torch.randn(N, 3, lowrank, generator=g).to(dtype).to(dev), w=(torch.randn(C, lowrank, generator=g) * 1.5).to(dev),
                        b=torch.randn(C, generator=g).to(dev), dy=None)
        return dict(x=(torch.randn(N, C, generator=g) * 6).to(dtype).to(dev), w=None, b=None, dy=torch.randn(N, C, generator=g).to(dtype).to(dev))

    def run(i):
        if lowrank:
            y = ops.gate_lowrank(i["x"], i["w"], i["b"], 16.0, None)
            return dict(y=y.detach(), dx=None)
        x = i["x"].requires_grad_()
        y = ops.gate_logsigmoid(x, 16.0, -0.2)
        (y.float() * i["dy"].float()).sum().backward()
        return dict(y=y.detach(), dx=x.grad)

    run = _kernel_run(run, "lina_gate_lowrank" if lowrank else "lina_gate_logsigmoid")
    return Op(f"gate-{'lowrank' if lowrank else 'logsigmoid'}-N{N}-C{C}-{_name(dtype)}", make, run, (N,),
              dict(x=0, w=None, b=None, dy=0), dict(y=0, dx=0))


def op_cross_entropy(N, V, dtype):
    """K14 ``cross_entropy``: per row the log-sum-exp and the loss (``lina_cross_entropy`` called through the backend as the
    forward of ``ops.cross_entropy`` calls it: the launcher keeps both tensors to itself) and the dlogits rows through
    ``ops.cross_entropy`` and autograd.  The mean loss is a scalar over all rows: shared, excluded.  The backward scales every
    row by dloss / (rows of the launch that count); ``run`` sends dloss = that count, read off the targets it is handed, so the
    scale is exactly 1 in any launch and a dlogits row is softmax - onehot, the row's own.  Targets stay as they are under
    the poisoned check.  An odd width: a row launched alone or in another slot starts at another alignment."""
    def make(dev):
        g = _gen(53 + N)
        tgt = torch.randint(0, V, (N,), generator=g)
        tgt[::5] = 1                                  # the ignored class
        return dict(logits=(torch.randn(N, V, generator=g) * 4).to(dtype).to(dev), target=tgt.to(dev))

    def run(i):
        lg, tgt = i["logits"], i["target"]
        n, be = lg.shape[0], ops.get_backend()
        lse, rows = _nan_like((n,), F32, lg.device), _nan_like((n,), F32, lg.device)
        ops._check(be.lib.lina_cross_entropy(ops._ptr(lg), ops._ptr(tgt), ops._ptr(lse), ops._ptr(rows), None, None, n, V,
                                             lg.stride(0), 0, 1, ops._dt(lg), be.stream(lg)))
        lg = lg.requires_grad_()
        loss = ops.cross_entropy(lg, tgt, ignore_index=1)
        count = (tgt != 1).sum().to(torch.float32)
        loss.backward(count.reshape(loss.shape))
        return dict(lse=lse, loss_row=rows, dlogits=lg.grad, loss=loss.detach())

    run = _kernel_run(run, "lina_cross_entropy")
    keep = lambda i: dict(target=i["target"])
    return Op(f"cross-entropy-N{N}-V{V}-{_name(dtype)}", make, run, (N,), dict(logits=0, target=0),
              dict(lse=0, loss_row=0, dlogits=0, loss=None), alt_ints=keep)


def op_short_conv(B, T, D, W, dtype):
    """K3 ``short_conv`` forward over B with a mask, prefilling a cache.  Unit: a batch row; causal over T."""
    def make(dev):
        g = _gen(2 + B + T)
        return dict(x=torch.randn(B, T, D, generator=g).to(dtype).to(dev), w=(torch.randn(D, 1, W, generator=g) * 0.5).to(dtype).to(dev),
                    bias=torch.randn(D, generator=g).to(dtype).to(dev), mask=(torch.rand(B, T, generator=g) > 0.2).float().to(dev))

    def run(i):
        b, dev = i["x"].shape[0], i["x"].device
        cache = torch.full((b, D, W), 7.0, dtype=dtype, device=dev)
        y = ops.short_conv(i["x"], i["w"], None, i["mask"], cache, "silu")
        y2 = ops.short_conv(i["x"], i["w"], i["bias"], None, None, None)
        return dict(y=y, cache=cache, y_bias=y2)

    t0s = tuple(t for t in (min(45, T - 2), 64) if 0 < t < T)
    return Op(f"short-conv-B{B}-T{T}-D{D}-W{W}-{_name(dtype)}", make, run, (B,), dict(x=0, w=None, bias=None, mask=0),
              dict(y=0, cache=0, y_bias=0), checks=("permutation", "poisoned", "subset", "time"),
              time_axes=dict(x=1, y=1, y_bias=1), t0s=t0s)


# ----------------------------------------------------------------------------- the tables
def _p(factory, *a, **kw):
    op = factory(*a, **kw)
    return pytest.param(op, id=op.name)


def _linear_forms(Ms, N, K, dtypes, forms=("rows", "packed")):
    out = []
    for form in forms:
        for M in Ms:
            for dtype in dtypes:
                out.append(_p(op_linear, M, N, K, dtype, form=form, resid=True))
        out.append(_p(op_linear, 17, N, K, dtypes[-1], ln=True, bias=True, form=form))
        out.append(_p(op_linear, 17, 96 if form == "rows" else 64, K, dtypes[0], ln=True, bias=True, swiglu=85 if form == "rows" else 37,
                      form=form))
    return out


def table(gpu):
    """The emulator list (``gpu`` False) or the device's full table."""
    K = 1024 if gpu else 64
    Kb = 1376 if gpu else 160
    t = []
    # projections
    t += _linear_forms((5, 17, 40), 40 if not gpu else 1024, K, (F32, BF16))
    t.append(_p(op_linear, 40, 33, Kb, BF16, bias=True, form="rows"))
    t += [_p(op_linear, 130, 70, 160, BF16, resid=True, form="tall", variant=v) for v in (0, 1, 2)]
    t += [_p(op_linear, 130, 56, 288, BF16, ln=True, bias=True, swiglu=40, form="tall", variant=v) for v in (0, 1, 2)]
    t += [_p(op_linear, 130, 48, 80, F32, ln=True, bias=True, resid=True, form="tall", variant=v) for v in (0, 2)]
    t += [_p(op_swiglu, 17, 85, dt) for dt in (F32, BF16)]
    # in-projection
    t += [_p(op_inproj, B, 64, 32, 48, dt, form=f) for f in ("rows", "packed", "prologue") for B, dt in ((5, F32), (17, BF16), (40, BF16))]
    t += [_p(op_inproj, 130, 96, 64, 128, BF16, form="tall", variant=v) for v in (0, 1, 2, 3)]
    t += [_p(op_inproj, 130, 48, 64, 64, F32, form="tall", variant=v) for v in (0, 3)]
    # K1d, K1d + K5, K5 over partials
    for fused in (False, True):
        t.append(_p(op_decode_update, 5, 4, 256, 128 if not gpu else 256, BF16, fused))
        t.append(_p(op_decode_update, 3, 2, 64, 64, F32, fused))
    # K1w
    wide = 256 if gpu else 64
    Bw = 3 if gpu else 2          # (b, h) grid 3 x 3 on the device, 2 x 3 on the emulator
    for window in (8, 1):
        for n_wg in (0, 3, Bw * 3 + 5):
            t.append(_p(op_decode_window, Bw, 3, wide, wide, BF16, F32, window, n_wg))
        t.append(_p(op_decode_window, Bw, 3, wide, wide, BF16, BF16, window, 3))
        t.append(_p(op_decode_window, Bw, 3, 64, 128, F32, F32, window, 0))
        t.append(_p(op_decode_window, 2, 3 if gpu else 2, 256 if gpu else 64, 512, BF16, F32, window, 0))
    t.append(_p(op_decode_window, Bw, 3, wide, wide, BF16, F32, 8, 0, packed=True))
    t.append(_p(op_decode_window, Bw, 3, wide, wide, BF16, F32, 8, 3, packed=True))
    # cross-attention
    t += [_p(op_cross, 5, 9, 64, F32), _p(op_cross, 17, 33, 256, BF16) if gpu else _p(op_cross, 17, 9, 256, BF16, parts=("spe", "pe")), _p(op_cross, 5, 13, 256, F32),
          _p(op_cross, 40, 70, 128, BF16) if gpu else _p(op_cross, 40, 9, 64, BF16, parts=("spe", "add"))]
    # picks, sampling, embedding
    t += [_p(op_argmax, 17, 4099 if gpu else 300, dt) for dt in (F32, BF16)]
    t += [_p(op_topk, 17, 300, 7, F32), _p(op_topk, 17, 1030 if gpu else 300, 100, BF16), _p(op_topk, 17, 300, 7, F32, hashed=True)]
    t += [_p(op_embed_sum, 2, 17, 2, 37, 64, F32), _p(op_embed_sum, 1, 5, 3, 37, 64, BF16)]
    t += [_p(op_pick, 17, 3, 70, 32, BF16, "greedy"), _p(op_pick, 5, 1, 70, 32, F32, "greedy"),
          _p(op_pick, 17, 3, 70, 32, BF16, "sample", n_sampled=0),
          _p(op_pick, 17, 3, 70, 32, BF16, "sample", n_sampled=2, steps=4 if gpu else 2),
          _p(op_pick, 5, 1, 50, 20, F32, "sample", n_sampled=1),
          _p(op_pick, 17, 4 if gpu else 2, 70, 64, BF16, "forced"), _p(op_pick, 5, 1, 70, 64, F32, "forced"),
          _p(op_pick, 17, 4 if gpu else 2, 70, 64, BF16, "forced", n_sampled=1, steps=4 if gpu else 3)]
    # K1 / K2
    T = 100 if gpu else 70
    Bk = 2 if gpu else 1          # the emulator takes seconds per 256 x 256 head
    t += [_p(op_gla, "fused_recurrent_gla", 2, 2, 37, 128, 64, F32, t0s=(20, 32)),
          _p(op_gla, "fused_recurrent_gla", 2, 2, 37 if gpu else 5, 256, 256, BF16, with_h0=False, t0s=(20, 32) if gpu else (3,)),
          _p(op_gla, "chunk_gla", 2, 2, 70, 64, 64, F32), _p(op_gla, "fused_chunk_gla", Bk, 2, 50, 128, 256, BF16, t0s=(45, 32)),
          _p(op_gla, "chunk_simple_gla", 2, 2, 70, 64, 64, F32), _p(op_gla, "chunk_simple_gla", 2, 2, 70, 64, 128, BF16, with_h0=False),
          _p(op_gla, "chunk_gla", 2, 4, T, 256, 256, BF16) if gpu else _p(op_gla, "chunk_gla", 2, 1, T, 256, 256, BF16),
          _p(op_gla, "chunk_gla", Bk, 2, T, 256, 256, BF16, with_h0=False),
          _p(op_gla, "chunk_gla", 2, 2, 70, 128, 128, BF16, subset_units="rows"),
          _p(op_gla, "chunk_gla", 2, 4, 70, 64, 64, BF16, subset_units="rows"),
          _p(op_gla, "chunk_gla", Bk, 2, T, 256, 256, BF16, nseg=3),
          _p(op_gla, "chunk_gla", 2, 4, 70, 64, 64, BF16, nseg=2, subset_units="rows"),
          _p(op_gla, "chunk_gla", Bk, 2, 100 if gpu else 40, 256, 512, BF16, dv512_one_launch=False, t0s=(45, 64) if gpu else (20, 32))]
    if gpu:       # what takes the emulator too long, or runs concurrently only on the device
        t += [_p(op_gla, "chunk_gla", 2, 2, 257, 256, 256, BF16, nseg=16),
              _p(op_gla, "chunk_gla", 1, 8, 100, 256, 256, BF16),
              _p(op_gla, "chunk_gla", 2, 2, 100, 256, 512, BF16, dv512_one_launch=True),
              _p(op_gla, "chunk_gla", 1, 8, 70, 256, 512, BF16, dv512_one_launch=True),
              _p(op_gla, "chunk_gla", 2, 16, 70, 64, 64, BF16, subset_units="rows")]
    else:
        t += [_p(op_gla, "chunk_gla", 1, 2, 65, 256, 256, BF16, nseg=16, t0s=(45, 64))]
    # K2b
    t += [_p(op_gla_bwd, 2, 2 if gpu else 1, 37, 64, 64, F32, "sweeps"), _p(op_gla_bwd, Bk, 2, 50 if gpu else 37, 128, 256, BF16, "sweeps"),
          _p(op_gla_bwd, 2, 2 if gpu else 1, 33 if not gpu else 100, 256, 256, BF16, "full", nseg=1),
          _p(op_gla_bwd, 2, 2, 150, 256, 256, BF16, "full", nseg=4) if gpu else _p(op_gla_bwd, 2, 2, 40, 128, 128, BF16, "full", nseg=2, subset_units="rows"),
          _p(op_gla_bwd, 2, 4, 70 if gpu else 40, 64, 64, BF16, "full", nseg=2, subset_units="rows")]
    # row-wise training ops
    t += [_p(op_layer_norm, 17, 320, F32), _p(op_layer_norm, 17, 128, BF16), _p(op_layer_norm, 5, 64, F32, resid=False),
          _p(op_rmsnorm_bwd, 17, 256, F32), _p(op_rmsnorm_bwd, 17, 256, BF16),
          _p(op_swiglu_gate, 17, 85, F32), _p(op_swiglu_gate, 17, 85, BF16), _p(op_swiglu_gate, 17, 128, BF16),
          _p(op_gate, 17, 244, F32), _p(op_gate, 17, 244, BF16), _p(op_gate, 17, 64, F32, lowrank=16), _p(op_gate, 17, 64, BF16, lowrank=7),
          _p(op_cross_entropy, 37, 131, F32), _p(op_cross_entropy, 17, 1027 if gpu else 131, BF16),
          _p(op_short_conv, 5, 70, 96, 4, F32), _p(op_short_conv, 3, 130 if gpu else 70, 96, 3, BF16)]
    names = [p.id for p in t]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return t


REARM = [(5, 32, BF16), (17, 64, F32), (40, 20, F32)]
