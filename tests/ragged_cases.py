"""Shared checks of ragged-text decoding (right-padded texts of different lengths in one batch): the three ragged
cross-attention launches against a float64 expression of the masked attention, and ``generate_batch(x_lens=...)`` row by row
against the same rows decoded alone.  `dev` = "cpu" (ops bound to the wave64 emulator) or "cuda" (the HIP library)."""
import torch

from kernel_cases import F64, assert_close
from lina_speech_amd import ops

LENS = (1, 7, 31, 32, 33)              # + T_txt itself


def ragged_lens(B, Tmax):
    pool = LENS + (Tmax,)
    if B == 1:
        return [33 if Tmax > 33 else Tmax]
    if B == 3:
        return [1, 33 if Tmax > 33 else Tmax, Tmax]
    return [pool[i % len(pool)] for i in range(B)]


def _ln(q, w, b, eps=1e-5):
    mu = q.mean(-1, keepdim=True)
    var = ((q - mu) ** 2).mean(-1, keepdim=True)
    return (q - mu) / torch.sqrt(var + eps) * w + b


def _launch(dev, dtype, q_lin, ln_w, ln_b, kk, vv, pe, x0, lens, scale, packed=False, att_log=None, step=None):
    """The three ragged launches of one cross-attention step (pos_net block left out: x_pos = xp).  Returns
    (scores, att [B,2,Tn], xp, x) -- or the packed forms unpacked."""
    B, Tn, d = kk.shape
    txt_len = torch.tensor(lens, dtype=torch.int32).to(dev)
    scores = torch.full((B, Tn), float("nan"), dtype=torch.float32, device=dev)
    ops.cross_scores_ragged(q_lin, ln_w, ln_b, 1e-5, kk, scores, scale, txt_len)
    att = torch.full((B, 2, 1, Tn), 7.0, dtype=dtype, device=dev)
    xp = torch.full((B, d), float("nan"), dtype=dtype, device=dev)
    xp_p = torch.zeros(ops.packed_numel(B, d), dtype=dtype, device=dev) if packed else None
    log_kw0, log_kw1 = {}, {}
    a0, a1 = att[:, 0, 0], att[:, 1, 0]
    if att_log is not None:
        a0, a1 = att_log[:, 0, 0], att_log[:, 1, 0]
        log_kw0 = log_kw1 = dict(att_step=step, att_step_stride=att_log.stride(2), att_steps=att_log.shape[2])
    ops.softmax_pe_rows_ragged(scores, a0, pe, xp, txt_len, xp_packed=xp_p, **log_kw0)
    x = x0.clone()
    if packed:
        x_p = ops.pack_rows(x0)
        ops.pe_softmax_weighted_rows_add_ragged(xp_p, pe, scale, a1, vv, x, txt_len, x_packed=x_p, xp_is_packed=True,
                                                **log_kw1)
        assert torch.equal(ops.unpack_rows(xp_p, B, d), xp), "packed copy of xp differs from the row-major xp"
        x = ops.unpack_rows(x_p, B, d)
    else:
        ops.pe_softmax_weighted_rows_add_ragged(xp, pe, scale, a1, vv, x, txt_len, **log_kw1)
    return scores, att[:, :, 0], xp, x


def check_ragged_kernels(dev, B, d, dtype, Tmax=64, shared_pe=False):
    """lina_cross_scores_ragged -> lina_softmax_pe_rows_ragged -> lina_pe_softmax_weighted_rows_add_ragged vs float64 torch of
    the masked attention (positions >= L_b left out); att rows exactly zero past L_b; row b bit-equal to the same row launched
    alone at T_txt = L_b; all lengths = T_txt on a shared table bit-equal to the uniform launches (d % 256 == 0); the packed
    operand forms equal to the row-major ones; the att-log form files the rows at the device step index."""
    g = torch.Generator().manual_seed(97 + B + d)
    mk = lambda *s_: torch.randn(*s_, generator=g).to(dtype).to(dev)
    lens = ragged_lens(B, Tmax)
    q_lin, kk, vv, x0 = mk(B, d), mk(B, Tmax, d), mk(B, Tmax, d), mk(B, d)
    ln_w = (1 + 0.1 * torch.randn(d, generator=g)).to(dtype).to(dev)
    ln_b = (0.1 * torch.randn(d, generator=g)).to(dtype).to(dev)
    pe = mk(Tmax, d) if shared_pe else mk(B, Tmax, d)
    scale = d ** -0.5
    kq = 32 if dtype == torch.bfloat16 else 16
    scores, att, xp, x = _launch(dev, dtype, q_lin, ln_w, ln_b, kk, vv, pe, x0, lens, scale)
    tol = 2e-2 if dtype == torch.bfloat16 else 1e-5
    c = lambda t: t.detach().cpu().to(F64)
    qn = _ln(c(q_lin), c(ln_w), c(ln_b)).to(dtype).to(F64)               # the LN output is rounded to the model dtype
    got, ref = {k: [] for k in ("sc", "a1", "xp", "a2", "x")}, {k: [] for k in ("sc", "a1", "xp", "a2", "x")}
    for b, L in enumerate(lens):                              # (compared over the whole batch: relative to max |ref|)
        peb = c(pe)[:L] if shared_pe else c(pe[b])[:L]
        sc2 = (c(xp[b]) @ peb.t()).to(dtype).to(F64) * scale
        for k, g_, r_ in (("sc", scores[b, :L], (c(kk[b, :L]) @ qn[b]) * scale),
                          ("a1", att[b, 0, :L], torch.softmax(c(scores[b, :L]), -1)),
                          ("xp", xp[b], c(att[b, 0, :L]) @ peb),
                          ("a2", att[b, 1, :L], torch.softmax(sc2, -1)),
                          ("x", x[b], c(x0[b]) + c(att[b, 1, :L]) @ c(vv[b, :L]))):
            got[k].append(c(g_))
            ref[k].append(r_)
        assert bool(torch.isnan(scores[b, L:].cpu()).all()), "scores past the row's text were written"
        assert float(att[b, :, L:].abs().max() if L < Tmax else 0.0) == 0.0, "att row not zero past the text"
    bf = dtype == torch.bfloat16
    for k, t, what in (("sc", 2e-3 if bf else 1e-5, "ragged cross scores"), ("a1", tol, "ragged softmax_pe_rows att"),
                       ("xp", tol, "ragged softmax_pe_rows xp"), ("a2", 3e-2 if bf else 1e-4, "ragged pe tail att"),
                       ("x", 3e-2 if bf else 1e-5, "ragged pe tail x")):
        assert_close(torch.cat(got[k]), torch.cat(ref[k]), t, what)
    # row b == the same row launched alone at T_txt = L_b (the ragged launch, and the uniform one where it exists)
    for b in sorted({0, B // 2, B - 1}):
        L = lens[b]
        peb = (pe[:L] if shared_pe else pe[b, :L]).contiguous()
        one = lambda t: t[b:b + 1, :L].contiguous()
        s1, a1, xp1, x1 = _launch(dev, dtype, q_lin[b:b + 1], ln_w, ln_b, one(kk), one(vv), peb, x0[b:b + 1], [L], scale)
        assert torch.equal(s1[0], scores[b, :L]) and torch.equal(a1[0], att[b, :, :L]), f"row {b}: scores / att differ alone"
        assert torch.equal(xp1[0], xp[b]) and torch.equal(x1[0], x[b]), f"row {b}: xp / x differ alone"
        if d % 256 == 0:
            su = torch.empty(1, L, dtype=torch.float32, device=dev)
            ops.cross_scores(q_lin[b:b + 1], ln_w, ln_b, 1e-5, one(kk), su, scale)
            au = torch.zeros(1, 2, 1, L, dtype=dtype, device=dev)
            xpu = torch.empty(1, d, dtype=dtype, device=dev)
            ops.softmax_pe_rows(su, au[:, 0, 0], peb, xpu)
            xu = x0[b:b + 1].clone()
            ops.pe_softmax_weighted_rows_add(xpu, peb, scale, au[:, 1, 0], one(vv), xu)
            assert torch.equal(su[0], scores[b, :L]) and torch.equal(au[0, :, 0], att[b, :, :L]), f"row {b} vs uniform at L_b"
            assert torch.equal(xpu[0], xp[b]) and torch.equal(xu[0], x[b]), f"row {b}: xp / x vs uniform launch at L_b"
    if d % kq == 0:                                                      # fragment-major xp / x
        _, att_p, xp_p, x_p = _launch(dev, dtype, q_lin, ln_w, ln_b, kk, vv, pe, x0, lens, scale, packed=True)
        assert torch.equal(att_p, att) and torch.equal(xp_p, xp) and torch.equal(x_p, x), "packed forms differ"
    # att-log form: rows filed at log[b, k, step[0], :], zeros past L_b; a step outside the log is dropped
    cap = 3
    log = torch.full((B, 2, cap, Tmax), 5.0, dtype=dtype, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    for t in (1, cap):
        step.fill_(t)
        before = log.clone()
        _, _, xp_l, x_l = _launch(dev, dtype, q_lin, ln_w, ln_b, kk, vv, pe, x0, lens, scale, att_log=log, step=step)
        assert torch.equal(xp_l, xp) and torch.equal(x_l, x)
        if t < cap:
            assert torch.equal(log[:, :, t], att), "att log row"
            before[:, :, t] = att
        assert torch.equal(log, before), "att log: something else was written"
    # every length = T_txt, one shared table: bit-equal to the uniform launches
    if d % 256 == 0:
        pes = pe if shared_pe else pe[0].contiguous()
        full = [Tmax] * B
        s_r, a_r, xp_r, x_r = _launch(dev, dtype, q_lin, ln_w, ln_b, kk, vv, pes, x0, full, scale)
        su = torch.empty(B, Tmax, dtype=torch.float32, device=dev)
        ops.cross_scores(q_lin, ln_w, ln_b, 1e-5, kk, su, scale)
        au = torch.zeros(B, 2, 1, Tmax, dtype=dtype, device=dev)
        xpu = torch.empty(B, d, dtype=dtype, device=dev)
        ops.softmax_pe_rows(su, au[:, 0, 0], pes, xpu)
        xu = x0.clone()
        ops.pe_softmax_weighted_rows_add(xpu, pes, scale, au[:, 1, 0], vv, xu)
        assert torch.equal(s_r, su) and torch.equal(a_r, au[:, :, 0]), "full lengths: scores / att differ from uniform"
        assert torch.equal(xp_r, xpu) and torch.equal(x_r, xu), "full lengths: xp / x differ from the uniform launches"


# ----------------------------------------------------------------------------- model level: generate_batch(x_lens=...)
RAGGED_LENS = (13, 40, 1, 64)


def ragged_texts(lens, Tmax, seed=3, pad=0):
    """[B, Tmax] random texts right-padded with ``pad`` (int, or "random": random ids in the padding)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(3, 256, (len(lens), Tmax), generator=g)
    for i, L in enumerate(lens):
        x[i, L:] = torch.randint(3, 256, (Tmax - L,), generator=g) if pad == "random" else pad
    return x


def tiny_model(dev, stop_boost=None):
    """The d = 64 golden model (ConvPos, one block each side): ``peak_logits`` (peaked, margin-rich greedy decodes) by default;
    ``stop_boost``: the golden weights with the stop token's head row scaled instead, so that rows stop early at different
    steps."""
    from model_cases import build_lina, golden_state_dict, load_golden, peak_logits
    model = build_lina()
    model.load_state_dict(golden_state_dict(load_golden("lina_d64.npz")), strict=True)
    if stop_boost is None:
        peak_logits(model)
    else:
        with torch.no_grad():
            model.logits_head.weight[0, 2] *= stop_boost
    return model.to(dev).eval()


def assert_rows_alone(got, alone, lens, rel, what):
    """Row i of the ragged call == ``alone[i]`` (the same text, trimmed, decoded with batch_size=1): tokens and stop flags
    over the alone run's steps, the cut's codes and shape exactly, attention rows within ``rel`` on [0, L_i) and exact zeros
    past it."""
    qs, atts, stops, cuts = got
    Tmax = atts.shape[-1]
    for i, (a, L) in enumerate(zip(alone, lens)):
        n = a[0].shape[-1]
        assert qs.shape[-1] >= n, f"{what}: the batch ended before row {i} stopped"
        assert torch.equal(qs[:, i, :n].cpu(), a[0][:, 0].cpu()), f"{what}: row {i} (L = {L}) tokens differ from its alone run"
        assert torch.equal(stops[i, :n].cpu(), a[2][0, :n].cpu()), f"{what}: row {i} stop flags differ"
        assert torch.equal(cuts[i][0].cpu(), a[3][0][0].cpu()), f"{what}: row {i} cut codes differ"
        assert cuts[i][1].shape == a[3][0][1].shape, f"{what}: row {i} cut shape {tuple(cuts[i][1].shape)}"
        err = float((atts[i, :, :n, :L].float().cpu() - a[1][0].float().cpu()).abs().max())
        record = max(float(a[1][0].abs().max()), 1e-30)
        assert err / record <= rel, f"{what}: row {i} attention log differs by {err / record:.2e}"
        if L < Tmax:
            assert float(atts[i, :, :, L:].abs().max()) == 0.0, f"{what}: row {i} attention log not zero past its text"


def check_ragged_generate(dev, rel=2e-5, n=12):
    """generate_batch(x [4, 64] right-padded, x_lens=(13, 40, 1, 64)): every row decodes as its text alone, on the device
    loop (one engine and the two-engine group), engine='fused', engine='module' and with a codec prompt (the teacher-forced
    prefill); the list form equals the padded form; lengths all = Tmax are the uniform call bit for bit."""
    model = tiny_model(dev)
    lens, Tmax = list(RAGGED_LENS), 64
    x = ragged_texts(lens, Tmax).to(dev)
    kw = dict(max_seqlen=n, k=1, first_greedy_quant=0, device=dev, force_max_seqlen=True)
    alone = [model.generate_batch(x[i:i + 1, :L], batch_size=1, **kw) for i, L in enumerate(lens)]
    got = model.generate_batch(x, batch_size=4, x_lens=lens, **kw)
    assert got[1].shape == (4, 2, n, Tmax)
    assert_rows_alone(got, alone, lens, rel, "device loop")
    from lina_speech_amd.decode import DecodeEngine, DecodeEngineGroup
    eng = next(reversed(model._decode_engines.values()))
    assert isinstance(eng, DecodeEngine) and eng._ragged
    # the cached ragged engine re-armed for other lengths (in place: lengths, tables, text side)
    lens2 = [64, 5, 33, 2]
    x2 = ragged_texts(lens2, Tmax, seed=8).to(dev)
    got2 = model.generate_batch(x2, batch_size=4, x_lens=torch.tensor(lens2), **kw)
    assert next(reversed(model._decode_engines.values())) is eng, "ragged engine not re-armed"
    alone2 = [model.generate_batch(x2[i:i + 1, :L], batch_size=1, **kw) for i, L in enumerate(lens2)]
    assert_rows_alone(got2, alone2, lens2, rel, "device loop, re-armed")
    # one row: the cached 1-row engine re-armed for another length rebuilds that row's table (ConvPos: per row at B = 1 too)
    ca = model.attentive_rnn.cross_att
    x1 = ragged_texts([Tmax], Tmax, seed=9).to(dev)
    eng1 = None
    for L in (13, 40):
        alone1 = model.generate_batch(x1[:, :L], batch_size=1, **kw)
        got1 = model.generate_batch(x1, batch_size=1, x_lens=[L], **kw)
        e = next(e for e in model._decode_engines.values() if getattr(e, "_ragged", False) and e.B == 1)
        assert eng1 is None or e is eng1, "the 1-row ragged engine was not re-armed"
        eng1 = e
        table = ca.pos_table_rows(torch.arange(Tmax, device=dev).unsqueeze(0), torch.tensor([L]))
        assert torch.equal(e.parts[0].pe, table), f"1-row engine: positional table not rebuilt for L = {L}"
        assert_rows_alone(got1, [alone1], [L], rel, f"one row, L = {L}")
    for what, extra in (("two engines", dict(n_engines=2)), ("fused", dict(engine="fused")),
                        ("module", dict(engine="module"))):
        got = model.generate_batch(x, batch_size=4, x_lens=lens, **extra, **kw)
        assert_rows_alone(got, alone, lens, rel, what)
        if what == "two engines":
            assert isinstance(next(reversed(model._decode_engines.values())), DecodeEngineGroup)
    # codec prompt: the prefill is the teacher-forced cached pass
    # (a prompt of B rows is taken as it is; one of fewer rows is broadcast and offset by 3 -- the reference's rule)
    prompt = torch.randint(3, 250, (1, 4, 3), generator=torch.Generator().manual_seed(4)).to(dev)
    alone_p = [model.generate_batch(x[i:i + 1, :L], batch_size=1, prompt=prompt[:, i:i + 1], **kw) for i, L in enumerate(lens)]
    got = model.generate_batch(x, batch_size=4, x_lens=lens, prompt=prompt, **kw)
    assert_rows_alone(got, alone_p, lens, rel, "codec prompt")
    # list form == padded form
    got_l = model.generate_batch([x[i, :L] for i, L in enumerate(lens)], batch_size=4, **kw)
    ref = model.generate_batch(x, batch_size=4, x_lens=lens, **kw)
    assert torch.equal(got_l[0], ref[0]) and torch.equal(got_l[1], ref[1]), "list form differs from the padded form"
    # every length = Tmax: the uniform call, bit for bit
    xf = ragged_texts([Tmax] * 4, Tmax, seed=5).to(dev)
    a = model.generate_batch(xf, batch_size=4, x_lens=[Tmax] * 4, **kw)
    b = model.generate_batch(xf, batch_size=4, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert not next(reversed(model._decode_engines.values()))._ragged, "full lengths must take the uniform engine"


def check_ragged_init_state(dev, rel=2e-5, n=10):
    """``init_state`` with ragged lengths: every row decodes as its text alone from the same start state -- on the device loop
    (built: DecodeEngine(x_lens=) + reset(state=); then the cached engine re-armed: reset(x_enc, state=, x_lens=)),
    engine='fused' and engine='module'.  The start state must change the decode (else the check would show nothing)."""
    model = tiny_model(dev)
    rnn = model.attentive_rnn
    lens, Tmax = list(RAGGED_LENS), 64
    x = ragged_texts(lens, Tmax, seed=15).to(dev)
    torch.manual_seed(12)
    params = rnn.get_init_state_tuning_params(lora=2, device=dev)

    def state(B):                                           # a fresh Cache per call (the module path updates it in place)
        with torch.no_grad():
            return rnn.get_state_from_params(params, B, scale=1.0)

    kw = dict(max_seqlen=n, k=1, first_greedy_quant=0, device=dev, force_max_seqlen=True)
    alone = [model.generate_batch(x[i:i + 1, :L], batch_size=1, init_state=state(1), **kw) for i, L in enumerate(lens)]
    plain = model.generate_batch(x, batch_size=4, x_lens=lens, **kw)
    for what, engine in (("device loop", None), ("device loop, re-armed", None), ("fused", "fused"), ("module", "module")):
        got = model.generate_batch(x, batch_size=4, x_lens=lens, init_state=state(4), engine=engine, **kw)
        assert_rows_alone(got, alone, lens, rel, f"init_state, {what}")
    assert not torch.equal(plain[1], got[1]), "the start state did not change the decode"


def check_ragged_stops(dev, rel=2e-5):
    """Rows that stop at different steps: row i's stop step and cut are those of its alone run (the batch runs until the
    last row stops; the stop test is the reference's per-step one)."""
    model = tiny_model(dev, stop_boost=6.0)
    lens, Tmax = list(RAGGED_LENS), 64
    x = ragged_texts(lens, Tmax, seed=1).to(dev)
    kw = dict(max_seqlen=24, k=1, first_greedy_quant=0, device=dev)
    alone = [model.generate_batch(x[i:i + 1, :L], batch_size=1, **kw) for i, L in enumerate(lens)]
    got = model.generate_batch(x, batch_size=4, x_lens=lens, stop_check_every=4, **kw)
    assert_rows_alone(got, alone, lens, rel, "early stop")
    assert got[0].shape[-1] == max(a[0].shape[-1] for a in alone), "the batch must end where its last row stops"
    assert min(a[0].shape[-1] for a in alone) < 24, "some row must stop early"


def check_ragged_pad_invariance(dev, n=10):
    """The token ids in the padding do not matter: greedy and sampled decodes give identical tokens and attention logs."""
    model = tiny_model(dev)
    lens, Tmax = list(RAGGED_LENS), 64
    xa, xb = ragged_texts(lens, Tmax, pad=0).to(dev), ragged_texts(lens, Tmax, pad="random").to(dev)
    assert torch.equal(torch.cat([xa[i, :L] for i, L in enumerate(lens)]), torch.cat([xb[i, :L] for i, L in enumerate(lens)]))
    for sampled in (False, True):
        kw = dict(max_seqlen=n, device=dev, force_max_seqlen=True, seed=11)
        kw.update(dict(k=20, first_greedy_quant=1, temp=0.9) if sampled else dict(k=1, first_greedy_quant=0))
        a = model.generate_batch(xa, batch_size=4, x_lens=lens, **kw)
        b = model.generate_batch(xb, batch_size=4, x_lens=lens, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), f"pad contents changed the decode (sampled={sampled})"


def check_ragged_errors(dev):
    """Bad lengths and bad forms raise ValueError; the A/B-only engine switches take no lengths."""
    import pytest
    from lina_speech_amd.decode import DecodeEngine
    model = tiny_model(dev)
    x = ragged_texts([5, 9], 9).to(dev)
    kw = dict(max_seqlen=2, k=1, first_greedy_quant=0, device=dev)
    for bad in ([5], [5, 9, 9], [0, 9], [5, 10], [5, -1]):
        with pytest.raises(ValueError):
            model.generate_batch(x, batch_size=2, x_lens=bad, **kw)
    with pytest.raises(ValueError):
        model.generate_batch(x[0], batch_size=2, x_lens=[5, 9], **kw)               # a 1-D x is one text for every row
    with pytest.raises(ValueError):
        model.generate_batch([x[0, :5], x[1]], batch_size=3, **kw)                  # list form: batch_size = len(x)
    with pytest.raises(ValueError):
        model.generate_batch([x[0, :5], x[1]], batch_size=2, x_lens=[5, 9], **kw)   # the list carries its lengths
    with pytest.raises(ValueError):
        model.generate_batch([x[0, :0], x[1]], batch_size=2, **kw)                  # an empty text
    x_enc = model.txt_encoder(model.txt_embed(x))
    for switch in (dict(cross="fused"), dict(cross_tail_fused=False)):
        with pytest.raises(ValueError):
            DecodeEngine(model, x_enc, batch_size=2, x_lens=[5, 9], **switch)
    eng = DecodeEngine(model, x_enc, batch_size=2)
    with pytest.raises(ValueError):
        eng.reset(x_lens=[5, 9])                                                    # a uniform engine takes no lengths


def encode_texts(model, x, lens):
    """The text side generate_batch(x_lens=) builds: the text encoder run with the reference's collate mask."""
    live = torch.arange(x.shape[1], device=x.device)[None, :] < torch.as_tensor(lens, device=x.device)[:, None]
    return model.txt_encoder(model.txt_embed(x), mask=live[:, None, :] & live[:, :, None])


def check_ragged_teacher_forced(dev, model, x, lens, rows, n_steps, bound):
    """A ragged engine and engines of single rows run alone (their texts trimmed) fed the SAME tokens through
    DecodeEngine.step (the ragged engine's greedy picks): logits per step within ``bound`` of max|logit| and equal greedy
    picks wherever the alone run's top-2 margin exceeds twice that bound.  Returns the worst relative error seen."""
    from lina_speech_amd.decode import DecodeEngine
    B = x.shape[0]
    with torch.inference_mode():
        eng = DecodeEngine(model, encode_texts(model, x, lens), batch_size=B, x_lens=lens)
        solo = {i: DecodeEngine(model, model.txt_encoder(model.txt_embed(x[i:i + 1, :lens[i]])), batch_size=1) for i in rows}
        emb = model.rvq_embed
        tok = torch.ones(model.n_quant, B, 1, dtype=torch.long, device=x.device)
        worst = 0.0
        for t in range(n_steps):
            y = emb.embed_sum(tok)                                              # [B, 1, d]
            lg, att = eng.step(y)
            picks = lg[:, 0].float().argmax(-1)                                 # [B, Q]
            for i in rows:
                lg1, att1 = solo[i].step(y[i:i + 1])
                ref = lg1[0, 0].float()
                err = float((lg[i, 0].float() - ref).abs().max() / ref.abs().max())
                worst = max(worst, err)
                assert err <= bound, f"step {t} row {i} (L = {lens[i]}): logits differ by {err:.2e} > {bound:.1e}"
                top2 = ref.topk(2, dim=-1).values
                margin = (top2[:, 0] - top2[:, 1]) / ref.abs().max()
                ok = margin > 2 * bound
                assert torch.equal(picks[i][ok], ref.argmax(-1)[ok]), f"step {t} row {i}: greedy pick differs"
                L = lens[i]
                assert float(att[i, :, :, L:].abs().max() if L < x.shape[1] else 0.0) == 0.0
            tok = picks.t().unsqueeze(-1).contiguous()
    return worst
