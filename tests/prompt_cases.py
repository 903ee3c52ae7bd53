"""Shared checks of codec prompts of different lengths in one batch: the forced token epilogue K6f (lina_pick_embed_forced)
against K6d / K6e and K6a on the same inputs, the forced configuration of the device loop against a per-step Python loop, and
``generate_batch(prompt=..., prompt_lens=...)`` row by row against the same rows decoded alone with their own excerpt.
`dev` = "cpu" (ops bound to the wave64 emulator) or "cuda" (the HIP library)."""
import ctypes
import functools

import pytest
import torch

from lina_speech_amd import ops
from ragged_cases import RAGGED_LENS, assert_rows_alone, ragged_texts, tiny_model

FORCE_LENS = (0, 2, 5, 1, 7)           # per row, cycled; 7 lies past the prompt's P = 5 and below P_cap
P, P_CAP, STEPS, L_VOCAB = 5, 64, 8, 256


def _buffers(dev, B, Q, d, dtype, packed, with_ctl):
    return dict(x=torch.full((B, d), float("nan"), dtype=dtype, device=dev),
                tok_log=torch.full((STEPS, Q, B), -1, dtype=torch.int64, device=dev),
                step=torch.zeros(1, dtype=torch.int64, device=dev),
                counter=torch.zeros(1, dtype=torch.int32, device=dev),
                x_p=torch.zeros(ops.packed_numel(B, d), dtype=dtype, device=dev) if packed else None,
                ctl=ops.new_loop_ctl(B, dev) if with_ctl else None)


def _step_logits(g, t, B, Q, dtype, dev):
    """Random logits; nobody picks the stop token by chance, the last row picks it at t = 2 and every row at t = 5."""
    logits = torch.randn(B, Q, L_VOCAB, generator=g).to(dtype)
    logits[:, :, 2] = -40.0
    if t == 2:
        logits[B - 1, :, 2] = 40.0
    if t == 5:
        logits[:, :, 2] = 40.0
    return logits.to(dev)


# (x_packed, loop_ctl, every length zero) of the forced launches that share one unforced reference launch per step
VARIANTS = ((False, False, False), (True, False, False), (False, True, False), (True, True, False), (True, True, True))


def check_pick_embed_forced(dev, B, Q, d, dtype, variants=VARIANTS, n_sampled=0, k=1, temp=1.0, seed=0):
    """K6f over t = 0 .. 7, each variant (with / without x_packed, with / without loop_ctl; lengths (0, 2, 5, 1, 7) cycled, or all
    zero) on its own set of buffers, next to ONE unforced launch per step (K6d, or K6e with the same seed) fed the same logits:
    token log, step, counter and control block exactly equal at every step; x_out[b] bit-equal to K6a on force_tok[t] for the
    rows with t < force_len[b] and to the unforced kernel's row otherwise; the packed copy equal to pack_rows(x_out).  Every
    length zero: every output bit-identical to the unforced kernel.  Sampled quantizers: the picks equal K6c / K6b launched
    separately at the same (seed, step), forced row or not."""
    g = torch.Generator().manual_seed(101 + B + 7 * Q + d)
    n_emb = L_VOCAB
    table = torch.randn(Q, n_emb, d, generator=g).to(dtype).to(dev)
    force_tok = torch.randint(0, n_emb, (P_CAP, Q, B), generator=g)          # defined past P as well
    if B > 1:
        force_tok[0, 0, 1], force_tok[1, Q - 1, 1] = n_emb + 5, -3             # clamped like K6a clamps them (row 1: length 2)
    force_tok = force_tok.to(dev)
    lens = [FORCE_LENS[b % len(FORCE_LENS)] for b in range(B)]
    force_len = torch.tensor(lens, dtype=torch.int32).to(dev)
    zero_len = torch.zeros(B, dtype=torch.int32).to(dev)
    r = _buffers(dev, B, Q, d, dtype, True, True)
    runs = [(_buffers(dev, B, Q, d, dtype, packed, with_ctl), zero) for packed, with_ctl, zero in variants]
    is_sampled = torch.arange(Q, device=dev).unsqueeze(0) < n_sampled
    n_forced = 0
    for t in range(STEPS):
        logits = _step_logits(g, t, B, Q, dtype, dev)
        if n_sampled:
            picks = torch.where(is_sampled, ops.topk_sample_rows(logits, k, temp, seed=seed, step=r["step"].clone()),
                                ops.argmax_rows(logits)).t().contiguous()                                    # [Q,B]
            ops.sample_pick_embed(logits, table, r["x"], r["tok_log"], r["step"], r["counter"], n_sampled, k, temp,
                                  seed=seed, x_packed=r["x_p"], loop_ctl=r["ctl"])
            assert torch.equal(r["tok_log"][t], picks)
        else:
            ops.greedy_pick_embed(logits, table, r["x"], r["tok_log"], r["step"], r["counter"], x_packed=r["x_p"],
                                  loop_ctl=r["ctl"])
        forced_x = ops.embed_sum(table, force_tok[t])                           # [B,d]
        want = r["x"].clone()
        for b in range(B):
            if t < lens[b]:
                want[b] = forced_x[b]
        inside = torch.tensor([t < n for n in lens])
        assert not bool(inside.any()) or not torch.equal(want[inside], r["x"][inside]), "the forced rows must differ"
        for f, zero in runs:
            what = f"step {t}, x_packed {f['x_p'] is not None}, loop_ctl {f['ctl'] is not None}, zero lengths {zero}"
            ops.pick_embed_forced(logits, table, f["x"], f["tok_log"], f["step"], f["counter"], force_tok,
                                  zero_len if zero else force_len, n_sampled, k, temp, seed=seed, x_packed=f["x_p"],
                                  loop_ctl=f["ctl"])
            assert int(f["step"]) == t + 1 and int(f["counter"]) == 0, what
            assert torch.equal(f["tok_log"], r["tok_log"]), f"{what}: token log differs from the unforced kernel's"
            if f["ctl"] is not None:
                assert torch.equal(f["ctl"], r["ctl"]), f"{what}: control block differs from the unforced kernel's"
            for b in range(B):                                                  # row by row: the message names the row
                assert torch.equal(f["x"][b], r["x"][b] if zero else want[b]), \
                    f"{what}, row {b}: " + ("not K6a of the forced tokens" if t < lens[b] and not zero
                                            else "differs from the unforced kernel")
            if f["x_p"] is not None:
                assert torch.equal(f["x_p"], ops.pack_rows(f["x"])), f"{what}: packed copy differs from pack_rows(x_out)"
                if zero:
                    assert torch.equal(f["x_p"], r["x_p"]), what
        n_forced += int(inside.sum())
    # (the last row stops at step 2 -- with one row that is every row --, all of them at step 5)
    assert r["ctl"].tolist()[:2] == [B, 2 if B == 1 else 5], "the stop flags must have fired"
    assert n_forced == sum(min(n, STEPS) for n in lens)


def check_pick_embed_forced_errors(dev):
    """Bad operands raise ValueError in the launcher; the C entry returns -1 / -2 with a message."""
    B, Q, d = 3, 2, 64
    b = _buffers(dev, B, Q, d, torch.float32, False, False)
    logits = torch.zeros(B, Q, L_VOCAB, device=dev)
    table = torch.zeros(Q, L_VOCAB, d, device=dev)
    ok_tok = torch.zeros(P_CAP, Q, B, dtype=torch.int64, device=dev)
    ok_len = torch.zeros(B, dtype=torch.int32, device=dev)
    call = lambda ft, fl: ops.pick_embed_forced(logits, table, b["x"], b["tok_log"], b["step"], b["counter"], ft, fl)
    call(ok_tok, ok_len)
    for ft, fl in ((None, ok_len), (ok_tok, None), (ok_tok.int(), ok_len), (ok_tok[:, :, :2].contiguous(), ok_len),
                   (ok_tok.permute(0, 2, 1).contiguous(), ok_len), (torch.zeros(P_CAP, B, Q, dtype=torch.int64, device=dev)
                                                                   .permute(0, 2, 1), ok_len),
                   (ok_tok[0], ok_len), (ok_tok, ok_len.long()), (ok_tok, ok_len[:2].contiguous()),
                   (ok_tok, torch.zeros(B, 1, dtype=torch.int32, device=dev))):
        with pytest.raises(ValueError):
            call(ft, fl)
    lib = ops.get_backend().lib
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    args = lambda ft, fl, Q_=Q, L_=L_VOCAB, pc=P_CAP: (one, Q_ * L_, one, one, z, one, one, one, z, B, Q_, L_, L_VOCAB, d, 8,
                                                      0, 1, 1.0, 0, ft, fl, pc, 0, z)
    for bad, word in ((args(z, one), b"force_tok"), (args(one, z), b"force_len"), (args(one, one, Q_=17), b"Q (<= 16)"),
                      (args(one, one, pc=0), b"P_cap")):
        assert lib.lina_pick_embed_forced(*bad) == -1 and word in lib.lina_last_error(), (word, lib.lina_last_error())
    assert lib.lina_pick_embed_forced(*args(one, one, L_=9000)) == -2 and b"L=9000" in lib.lina_last_error()


# ----------------------------------------------------------------------------- engine: the forced loop configuration
def _python_forced_loop(eng, model, toks, lens, n):
    """The reference's loop body with a p_len per row, one ``engine(y, t)`` call per token."""
    emb = model.rvq_embed
    Q, B, Pn = toks.shape
    lens_t = torch.as_tensor(lens, device=toks.device)
    y = emb.embed_sum(torch.ones(Q, B, 1, dtype=torch.long, device=toks.device))
    qs, atts = [], []
    for t in range(n):
        logits, att = eng(y, t)
        pick = ops.argmax_rows(logits[:, 0]).t().contiguous().unsqueeze(-1)             # [Q,B,1]
        qs.append(pick)
        atts.append(att)
        y = emb.embed_sum(pick)
        if t < Pn:
            y = torch.where((t < lens_t)[:, None, None], emb.embed_sum(toks[:, :, [t]]), y)
    return torch.cat(qs, dim=2), torch.cat(atts, dim=2)


def check_forced_engine(dev, rel=2e-5, n=10):
    """DecodeEngine.begin_greedy(forced=): tokens and attention log of the forced loop equal a Python loop over
    ``engine(y, t)`` with the per-row rule; other lengths re-arm the captured loop; a prompt longer than P_cap rebuilds it; the
    unforced loop gives afterwards what it gave before."""
    from lina_speech_amd.decode import DecodeEngine
    model = tiny_model(dev)
    B, Q = 4, model.n_quant
    x = ragged_texts([16] * B, 16, seed=2).to(dev)
    g = torch.Generator().manual_seed(6)
    toks = torch.randint(3, 250, (Q, B, 6), generator=g).to(dev)
    with torch.inference_mode():
        eng = DecodeEngine(model, model.txt_encoder(model.txt_embed(x)), batch_size=B)
        before = eng.run_greedy(n, record_att=True)
        plain_loop = eng._loop

        def run(tokens, lens):
            eng.reset()
            eng.begin_greedy(n, log_att=True, forced=(tokens, lens))
            eng.greedy_steps(n)
            got = eng.greedy_tokens(), eng.logged_atts()
            eng.reset()
            ref = _python_forced_loop(eng, model, tokens, lens, n)
            assert torch.equal(got[0], ref[0]), f"forced loop, lengths {lens}: tokens differ from the per-step loop"
            err = float((got[1].float() - ref[1].float()).abs().max() / ref[1].float().abs().max())
            assert err <= rel, f"forced loop, lengths {lens}: attention log differs by {err:.2e}"
            return got

        got = run(toks, [0, 3, 6, 1])
        loop = eng._loop
        assert loop.forced and loop is not plain_loop and loop.p_cap == 64
        assert not torch.equal(got[0], before[0]), "the forced tokens did not change the decode"
        graph1 = loop.graph1
        run(toks, torch.tensor([3, 0, 2, 6]))
        assert eng._loop is loop and loop.graph1 is graph1, "other lengths must re-arm the captured loop"
        if dev == "cuda":
            assert graph1 is not None
        long_toks = torch.randint(3, 250, (Q, B, 70), generator=g).to(dev)
        run(long_toks, [70, 0, 9, 2])
        assert eng._loop is not loop and eng._loop.p_cap == 128, "a prompt longer than P_cap must rebuild the loop"
        for bad in ([0, 3, 6], [0, 3, 7, 1], [0, -1, 6, 1]):
            with pytest.raises(ValueError):
                eng.begin_greedy(n, forced=(toks, bad))
        with pytest.raises(ValueError):
            eng.begin_greedy(n, forced=(toks[:, :2], [0, 1]))
        eng.reset()
        after = eng.run_greedy(n, record_att=True)
        assert eng._loop is plain_loop, "the unforced loop must be the one captured before"
        assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1]), "the unforced loop changed"


# ----------------------------------------------------------------------------- model: generate_batch(prompt_lens=...)
P_MODEL = 6
PROMPT_LENS = ((0, 3, 6, 1), (2, 3, 6, 4))     # the second: min > 0, i.e. prefill of 3 positions, then the forced loop


def prompt_tokens(Q, B, Pn, seed=4):
    return torch.randint(3, 250, (Q, B, Pn), generator=torch.Generator().manual_seed(seed))


def _kw(dev, n=12):
    return dict(max_seqlen=n, k=1, first_greedy_quant=0, device=dev, force_max_seqlen=True)


def alone_runs(model, x, lens, prompt, plens, **kw):
    """Row i as the one-prompt form decodes it: its text trimmed, its own excerpt (none for length 0), batch_size = 1."""
    return [model.generate_batch(x[i:i + 1, :L], batch_size=1, prompt=prompt[:, i:i + 1, :p] if p else None, **kw)
            for i, (L, p) in enumerate(zip(lens, plens))]


@functools.lru_cache(maxsize=None)
def _shared(dev):
    """The tiny model, its ragged texts, one padded prompt and the alone runs of both length sets: computed once per device
    and left unchanged."""
    model = tiny_model(dev)
    lens = list(RAGGED_LENS)
    x = ragged_texts(lens, 64).to(dev)
    prompt = prompt_tokens(model.n_quant, 4, P_MODEL).to(dev)
    alone = {pl: alone_runs(model, x, lens, prompt, pl, **_kw(dev)) for pl in PROMPT_LENS}
    return model, lens, x, prompt, alone


def _same(a, b, what):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), what
    for ca, cb in zip(a[3], b[3]):
        assert torch.equal(ca[0], cb[0]) and torch.equal(ca[1], cb[1]), what


def check_prompt_rows_alone(dev, engine=None, rel=1e-4):
    """Every row of the batched call equals its alone run -- tokens, stop flags and cut codes exactly, attention rows within
    ``rel`` (the alone run prefills p_i + 1 positions with the chunk scan, the batch steps some of them)."""
    model, lens, x, prompt, alone = _shared(dev)
    for pl in PROMPT_LENS:
        got = model.generate_batch(x, batch_size=4, x_lens=lens, prompt=prompt, prompt_lens=pl, engine=engine, **_kw(dev))
        assert got[0].shape[-1] == 12
        assert_rows_alone(got, alone[pl], lens, rel, f"prompt_lens {pl}, engine {engine}")
        if engine is None:
            eng = next(reversed(model._decode_engines.values()))
            assert eng._loop.forced, "the device loop must have run its forced configuration"


def check_prompt_list_form(dev):
    """A list of B prompts [Q, p_i] == the padded form with prompt_lens, bit for bit (and prompt_lens as a LongTensor)."""
    model, lens, x, prompt, _ = _shared(dev)
    for pl in PROMPT_LENS:
        ref = model.generate_batch(x, batch_size=4, x_lens=lens, prompt=prompt, prompt_lens=torch.tensor(pl), **_kw(dev))
        got = model.generate_batch(x, batch_size=4, x_lens=lens, prompt=[prompt[:, i, :p] for i, p in enumerate(pl)],
                                   **_kw(dev))
        _same(got, ref, f"list form differs from the padded form ({pl})")


def check_prompt_init_state(dev, rel=1e-4, n=10):
    """``init_state`` together with ragged texts and ragged prompts: rows equal alone from the same start state, on the device
    loop (built, then re-armed), engine='fused' and engine='module'."""
    model, lens, x, prompt, _ = _shared(dev)
    rnn = model.attentive_rnn
    torch.manual_seed(12)
    params = rnn.get_init_state_tuning_params(lora=2, device=dev)

    def state(B):
        with torch.no_grad():
            return rnn.get_state_from_params(params, B, scale=1.0)

    kw = _kw(dev, n)
    pl = PROMPT_LENS[1]
    alone = [model.generate_batch(x[i:i + 1, :L], batch_size=1, prompt=prompt[:, i:i + 1, :p], init_state=state(1), **kw)
             for i, (L, p) in enumerate(zip(lens, pl))]
    plain = model.generate_batch(x, batch_size=4, x_lens=lens, prompt=prompt, prompt_lens=pl, **kw)
    for what, engine in (("device loop", None), ("device loop, re-armed", None), ("fused", "fused"), ("module", "module")):
        got = model.generate_batch(x, batch_size=4, x_lens=lens, prompt=prompt, prompt_lens=pl, init_state=state(4),
                                   engine=engine, **kw)
        assert_rows_alone(got, alone, lens, rel, f"init_state, {what}")
    assert not torch.equal(plain[1], got[1]), "the start state did not change the decode"


def check_prompt_pad_invariance(dev):
    """The token ids past each row's prompt length do not matter: zeros against random ids, bit-identical returns."""
    model, lens, x, prompt, _ = _shared(dev)
    for pl in PROMPT_LENS:
        zeros, rand = prompt.clone(), prompt.clone()
        for i, p in enumerate(pl):
            zeros[:, i, p:] = 0
            rand[:, i, p:] = torch.randint(3, 250, (prompt.shape[0], P_MODEL - p), generator=torch.Generator().manual_seed(i))
        for engine in (None, "module"):
            a = model.generate_batch(x, batch_size=4, x_lens=lens, prompt=zeros, prompt_lens=pl, engine=engine, **_kw(dev))
            b = model.generate_batch(x, batch_size=4, x_lens=lens, prompt=rand, prompt_lens=pl, engine=engine, **_kw(dev))
            _same(a, b, f"pad contents of the prompt changed the decode ({pl}, engine {engine})")


def check_prompt_equal_lengths(dev, dtype=torch.float32, B=4, p=3):
    """Lengths all equal to p < P: bit-identical to the uniform call with prompt[:, :, :p] (texts of one length: the uniform
    engine).  Lengths all equal to P: the uniform path itself -- no forced loop is built."""
    model = tiny_model(dev).to(dtype)
    x = ragged_texts([32] * B, 32, seed=7).to(dev)
    prompt = prompt_tokens(model.n_quant, B, P_MODEL, seed=9).to(dev)
    kw = _kw(dev)
    ref = model.generate_batch(x, batch_size=B, prompt=prompt[:, :, :p].contiguous(), n_engines=1, **kw)
    got = model.generate_batch(x, batch_size=B, prompt=prompt, prompt_lens=[p] * B, **kw)
    _same(got, ref, f"equal lengths {p} < P differ from the uniform call (B = {B}, {dtype})")
    eng = next(reversed(model._decode_engines.values()))
    assert eng._loop.forced
    model.clear_decode_cache()
    full = model.generate_batch(x, batch_size=B, prompt=prompt, prompt_lens=[P_MODEL] * B, **kw)
    eng = next(reversed(model._decode_engines.values()))
    assert not any(L.forced for L in eng._loops.values()), "lengths all = P must take the uniform path"
    _same(full, model.generate_batch(x, batch_size=B, prompt=prompt, **kw), "lengths all = P differ from the uniform call")
    model.clear_decode_cache()


STOP_P, STOP_LENS = 16, (0, 16, 5, 11)


def check_prompt_stops(dev, rel=1e-4):
    """A stop-boosted model: a row that picks the stop token while still forced is flagged at that step, as in its alone run,
    and the call ends at the reference's step (the last row's stop) with ``stop_check_every`` 1 and 16."""
    model = tiny_model(dev, stop_boost=6.0)
    lens = list(RAGGED_LENS)
    x = ragged_texts(lens, 64, seed=1).to(dev)
    prompt = prompt_tokens(model.n_quant, 4, STOP_P, seed=13).to(dev)
    kw = dict(max_seqlen=24, k=1, first_greedy_quant=0, device=dev)
    alone = alone_runs(model, x, lens, prompt, STOP_LENS, **kw)
    first_stop = [int(a[2][0].argmax()) for a in alone]                     # (the closing column of ones bounds it)
    assert any(s < p for s, p in zip(first_stop, STOP_LENS)), f"no row stops inside its prompt: {first_stop}"
    for every in (1, 16):
        got = model.generate_batch(x, batch_size=4, x_lens=lens, prompt=prompt, prompt_lens=STOP_LENS,
                                   stop_check_every=every, **kw)
        assert_rows_alone(got, alone, lens, rel, f"early stop, stop_check_every={every}")
        assert got[0].shape[-1] == max(a[0].shape[-1] for a in alone), "the batch must end where its last row stops"


def check_prompt_errors(dev):
    """Every argument error of generate_batch(prompt_lens=...)."""
    model, lens, x, prompt, _ = _shared(dev)
    kw = dict(max_seqlen=2, k=1, first_greedy_quant=0, device=dev, x_lens=lens)
    for bad in ([1, 2, 3], [1, 2, 3, 4, 5], [0, 7, 1, 1], [0, -1, 1, 1], torch.tensor([[0, 1, 2, 3]])):
        with pytest.raises(ValueError):
            model.generate_batch(x, batch_size=4, prompt=prompt, prompt_lens=bad, **kw)
    rows = [prompt[:, i, :p] for i, p in enumerate(PROMPT_LENS[0])]
    with pytest.raises(ValueError):
        model.generate_batch(x, batch_size=4, prompt=rows, prompt_lens=list(PROMPT_LENS[0]), **kw)   # the list carries its lengths
    with pytest.raises(ValueError):
        model.generate_batch(x, batch_size=4, prompt=rows[:3], **kw)                                 # list form: B = len(prompt)
    with pytest.raises(ValueError):
        model.generate_batch(x, batch_size=4, prompt=None, prompt_lens=[0, 1, 2, 3], **kw)           # lengths of nothing
    with pytest.raises(ValueError):
        model.generate_batch(x, batch_size=4, prompt=prompt[:, :1], prompt_lens=[1], **kw)           # the one-prompt form
    with pytest.raises(ValueError):
        model.generate_batch(x, batch_size=4, prompt=prompt[:, :1], prompt_lens=[0, 1, 2, 3], **kw)
    model.spk_encoder = torch.nn.Identity()
    try:
        with pytest.raises(NotImplementedError):
            model.generate_batch(x, batch_size=4, prompt=prompt, prompt_lens=[0, 1, 2, 3], **kw)
    finally:
        model.spk_encoder = None
