"""Shared checks of queue decoding (``LinaModel.generate_queue`` / ``generate_stream``: finished decode rows are re-armed with the
next queued text between two graph replays): K6g ``lina_rows_rearm`` against torch index ops inside guard bands, and every
utterance of a queue against the same text decoded alone.  `dev` = "cpu" (ops bound to the wave64 emulator) or "cuda"."""
import ctypes

import pytest
import torch

import ragged_cases as RC
from guard import GuardArena
from lina_speech_amd import ops

R = ops.LOOP_CTL_ROWS


# ----------------------------------------------------------------------------- K6g
REARM_B = 5
REARM_ROWS = {1: [3], 3: [4, 0, 2], 5: [2, 0, 4, 1, 3]}
SEG_ROW_BYTES = (16, 48, 4112)


def check_rows_rearm(dev, n, dtype, d, packed, flagged):
    """One K6g launch on B = 5 rows, ``n`` of them listed (in no order): state segments of 16, 48 and 4112 bytes per row (fp32 and
    bf16 states side by side), the start embedding into x_out (and the fragment-major copy == ops.pack_rows of the row-major
    result), the stop bookkeeping with ``flagged`` in {"none", "some", "all"} of the listed rows flagged (and, where a row is
    left over, an unlisted one flagged too), the text lengths.  Everything else bit-unchanged; no guard band byte changed."""
    B = REARM_B
    rows = REARM_ROWS[n]
    others = [b for b in range(B) if b not in rows]
    g = torch.Generator().manual_seed(1000 * n + d + len(flagged))
    arena = GuardArena(dev)
    segs = []
    for st_dtype in (torch.float32, torch.bfloat16):
        for rb in SEG_ROW_BYTES:
            cols = rb // torch.empty(0, dtype=st_dtype).element_size()
            shape = (B, cols) if rb < 4112 else (B, 2, cols // 2)                 # (a [B, H, ...] state: rows stay contiguous)
            segs.append(arena.place(torch.randn(*shape, generator=g).to(st_dtype)))
    table = ops.RearmTable(segs, B)
    assert table.row_bytes_host.tolist() == list(SEG_ROW_BYTES) * 2
    table.ptr, table.row_bytes = arena.place(table.ptr), arena.place(table.row_bytes)
    y_start = arena.place(torch.randn(d, generator=g).to(dtype))
    x0 = torch.randn(B, d, generator=g).to(dtype)
    x_out = arena.place(x0)
    x_pk = arena.place(ops.pack_rows(x0)) if packed else None
    flags = torch.zeros(B, dtype=torch.int32)
    if flagged == "some":
        flags[rows[0]] = 1
    elif flagged == "all":
        flags[rows] = 1
    if others:
        flags[others[-1]] = 1                                                     # an unlisted row that has stopped stays so
    ctl0 = torch.cat([torch.tensor([int(flags.sum()), 7, 0x1234, -5], dtype=torch.int32), flags])
    ctl = arena.place(ctl0)
    txt0 = torch.arange(10, 10 + B, dtype=torch.int32)
    txt_len = arena.place(txt0)
    new_len = arena.place(torch.arange(1, n + 1, dtype=torch.int32))
    rows_t = arena.place(torch.tensor(rows, dtype=torch.int32))
    before = [s.clone() for s in segs]
    ops.rows_rearm(rows_t, table, y_start, x_out, x_packed=x_pk, loop_ctl=ctl, txt_len=txt_len, new_len=new_len)
    idx = torch.tensor(rows, device=dev)
    for s, s0 in zip(segs, before):
        want = s0.clone()
        want.index_fill_(0, idx, 0)
        assert torch.equal(s.view(torch.uint8), want.view(torch.uint8)), "state segment: listed rows not zero or others changed"
    want_x = x0.to(dev).clone()
    want_x.index_copy_(0, idx, y_start.unsqueeze(0).expand(n, -1).contiguous())
    assert torch.equal(x_out.view(torch.uint8), want_x.view(torch.uint8)), "x_out"
    if packed:
        assert torch.equal(x_pk, ops.pack_rows(want_x)), "x_out_packed differs from pack_rows of the row-major result"
    want_ctl = ctl0.clone()
    n_set = int(flags[rows].sum())
    want_ctl[0] -= n_set
    want_ctl[1] = -1
    want_ctl[R + torch.tensor(rows)] = 0
    assert torch.equal(ctl.cpu(), want_ctl), f"loop_ctl {ctl.cpu().tolist()} != {want_ctl.tolist()}"
    want_txt = txt0.clone()
    want_txt[torch.tensor(rows)] = torch.arange(1, n + 1, dtype=torch.int32)
    assert torch.equal(txt_len.cpu(), want_txt), "txt_len"
    assert torch.equal(rows_t.cpu(), torch.tensor(rows, dtype=torch.int32)) and torch.equal(
        new_len.cpu(), torch.arange(1, n + 1, dtype=torch.int32)), "an input was written"
    arena.check()


def check_rows_rearm_errors(dev):
    """Bad arguments come back as LINA_ERR_ARG (-1) and launch nothing: a null table, a row size that is no multiple of 16,
    n outside [1, B], txt_len without new_len; the launcher refuses a segment whose rows are not 16-byte multiples."""
    lib = ops.get_backend().lib
    B, d = 3, 64
    seg = torch.ones(B, 4, dtype=torch.float32, device=dev)
    table = ops.RearmTable([seg], B)
    rows = torch.tensor([1], dtype=torch.int32, device=dev)
    y = torch.zeros(d, device=dev)
    x = torch.ones(B, d, device=dev)
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    z = ctypes.c_void_p(0)
    good = dict(rows=p(rows), n=1, B=B, ptr=p(table.ptr), rb=p(table.row_bytes), rbh=p(table.row_bytes_host), n_seg=1,
                y=p(y), x=p(x), xp=z, d=d, ctl=z, txt=z, new=z)

    def call(**kw):
        a = {**good, **kw}
        return lib.lina_rows_rearm(a["rows"], a["n"], a["B"], a["ptr"], a["rb"], a["rbh"], a["n_seg"], a["y"], a["x"], a["xp"],
                                   a["d"], a["ctl"], a["txt"], a["new"], 0, z)

    bad_size = torch.tensor([24], dtype=torch.int64)
    for kw, word in ((dict(ptr=z), b"null segment table"), (dict(rb=z), b"null segment table"),
                     (dict(rbh=z), b"null segment table"), (dict(rbh=p(bad_size)), b"multiple of 16"),
                     (dict(n=0), b"n=0"), (dict(n=B + 1), b"n=4"), (dict(rows=z), b"null"),
                     (dict(txt=p(rows)), b"new_len"), (dict(d=6), b"multiple of 4")):
        assert call(**kw) == -1 and word in lib.lina_last_error(), (kw, lib.lina_last_error())
    assert bool((seg == 1).all()) and bool((x == 1).all()), "a rejected call wrote something"
    assert call() == 0
    if dev == "cuda":
        torch.cuda.synchronize()
    assert seg[:, 0].tolist() == [1.0, 0.0, 1.0] and x[:, 0].tolist() == [1.0, 0.0, 1.0]
    with pytest.raises(ValueError):
        ops.RearmTable([torch.zeros(B, 6, dtype=torch.float32, device=dev)], B)     # 24-byte rows
    with pytest.raises(ValueError):
        ops.rows_rearm(rows.to(torch.int64), table, y, x)


# ----------------------------------------------------------------------------- model level
QUEUE_LENS = (13, 40, 1, 64, 7, 33, 64, 2, 21, 50)
QUEUE_CAPS = (5, 24, 9, 17, 40, 3, 12, 33, 8, 21)
GREEDY = dict(k=1, first_greedy_quant=0)

_SHARED = {}


def queue_texts():
    x = RC.ragged_texts(list(QUEUE_LENS), 64, seed=31)
    return [x[i, :L].clone() for i, L in enumerate(QUEUE_LENS)]


def stop_case(dev):
    """(stop-boosted model, texts, alone runs at max_seqlen = 48): computed once per device and shared, never modified."""
    key = ("stop", dev)
    if key not in _SHARED:
        model = RC.tiny_model(dev, stop_boost=3.0)
        texts = [t.to(dev) for t in queue_texts()]
        alone = [model.generate_batch(t, batch_size=1, max_seqlen=48, device=dev, stop_check_every=8, **GREEDY) for t in texts]
        _SHARED[key] = (model, texts, alone)
    return _SHARED[key]


def caps_case(dev):
    """(peaked model -- it never stops --, texts, alone runs at max_seqlen = cap_i)."""
    key = ("caps", dev)
    if key not in _SHARED:
        model = RC.tiny_model(dev)
        texts = [t.to(dev) for t in queue_texts()]
        alone = [model.generate_batch(t, batch_size=1, max_seqlen=c, device=dev, **GREEDY) for t, c in zip(texts, QUEUE_CAPS)]
        _SHARED[key] = (model, texts, alone)
    return _SHARED[key]


def assert_equals_alone(got, alone, rel, what, ids=None):
    """``got[j]`` = (codes, att) of utterance ids[j] == ``cuts[0]`` of its alone run ``alone[j]``: codes and att shape exactly, att
    values within ``rel`` of the alone run's max."""
    assert len(got) == len(alone)
    for j, ((codes, att), a) in enumerate(zip(got, alone)):
        i = j if ids is None else ids[j]
        ref_codes, ref_att = a[3][0]
        assert codes.shape == ref_codes.shape and torch.equal(codes.cpu(), ref_codes.cpu()), \
            f"{what}: utterance {i} codes {tuple(codes.shape)} differ from its alone run {tuple(ref_codes.shape)}"
        assert att.shape == ref_att.shape, f"{what}: utterance {i} att shape {tuple(att.shape)} != {tuple(ref_att.shape)}"
        err = float((att.float().cpu() - ref_att.float().cpu()).abs().max()) if att.numel() else 0.0
        scale = max(float(ref_att.float().abs().max()) if ref_att.numel() else 0.0, 1e-30)
        print(f"{what}: utterance {i}: att err / max = {err / scale:.2e}")
        assert err / scale <= rel, f"{what}: utterance {i} attention differs by {err / scale:.2e} > {rel:.0e}"


def alone_steps(alone):
    return [int(a[0].shape[-1]) for a in alone]


def stop_queue_run(dev, B, stop_check_every):
    """generate_queue of the stop case: computed once per (device, B, stop_check_every) and shared, never modified."""
    key = ("run", dev, B, stop_check_every)
    if key not in _SHARED:
        model, texts, _ = stop_case(dev)
        _SHARED[key] = model.generate_queue(texts, batch_size=B, max_seqlen=48, stop_check_every=stop_check_every, device=dev,
                                            **GREEDY)
    return _SHARED[key]


def check_queue_stops(dev, B, stop_check_every, rel=2e-5):
    """Rows stop at different steps and are refilled while their neighbours are mid-utterance: every result == its alone run."""
    model, texts, alone = stop_case(dev)
    steps = alone_steps(alone)
    assert len(set(steps)) > 1 and max(steps) < 48, f"the alone runs must stop early at different steps: {steps}"
    got = stop_queue_run(dev, B, stop_check_every)
    assert_equals_alone(got, alone, rel, f"stops, B = {B}, every {stop_check_every}")


def check_queue_caps(dev, rel=2e-5):
    """A model that never stops, a step cap per utterance (3 .. 40: several check intervals), B = 3: results == the alone runs at
    max_seqlen = cap_i, and the log ring (64 steps here) wrapped at least once."""
    model, texts, alone = caps_case(dev)
    assert alone_steps(alone) == list(QUEUE_CAPS)
    got = model.generate_queue(texts, batch_size=3, max_seqlen=list(QUEUE_CAPS), stop_check_every=8, device=dev, **GREEDY)
    assert_equals_alone(got, alone, rel, "caps")
    eng = next(reversed(model._decode_engines.values()))
    assert eng.serve_cap in (64, 128) and eng.serve_cap % eng.serve_every == 0
    assert eng.ring_wraps >= 1, f"the ring of {eng.serve_cap} steps never wrapped"


def check_queue_invariance(dev, rel=2e-5):
    """Permuting the queue permutes the results; B = 1; N < B; N = 0; a second call reuses the cached engine."""
    model, texts, alone = stop_case(dev)
    kw = dict(max_seqlen=48, device=dev, **GREEDY)
    base = stop_queue_run(dev, 4, 16)
    perm = [7, 2, 9, 0, 5, 3, 8, 1, 6, 4]
    got = model.generate_queue([texts[i] for i in perm], batch_size=4, **kw)
    eng = next(reversed(model._decode_engines.values()))
    for j, i in enumerate(perm):
        assert torch.equal(got[j][0], base[i][0]) and torch.equal(got[j][1], base[i][1]), f"permuted queue: utterance {i} differs"
    assert_equals_alone(got, [alone[i] for i in perm], rel, "permuted", ids=perm)
    few = sorted(model.generate_stream(texts[4:6], batch_size=4, max_text_len=64, **kw), key=lambda r: r[0])   # N < B
    assert next(reversed(model._decode_engines.values())) is eng, "the cached engine was not reused"
    assert [r[0] for r in few] == [0, 1], "generate_stream must yield every utterance once"
    assert_equals_alone([r[1:] for r in few], alone[4:6], rel, "N < B, generate_stream", ids=[4, 5])
    one = model.generate_queue(texts[1:4], batch_size=1, max_text_len=64, **kw)
    assert_equals_alone(one, alone[1:4], rel, "B = 1", ids=[1, 2, 3])
    assert model.generate_queue([], batch_size=4, **kw) == []


def check_queue_sampled(dev):
    """Sampled mode: two calls with one seed are identical, another seed differs, every length is within its cap."""
    model, texts, _ = stop_case(dev)
    caps = [12, 5, 9, 12, 3, 12, 7, 12, 6, 12]
    kw = dict(batch_size=3, max_seqlen=caps, k=20, first_greedy_quant=1, device=dev)
    a = model.generate_queue(texts, seed=5, **kw)
    b = model.generate_queue(texts, seed=5, **kw)
    c = model.generate_queue(texts, seed=6, **kw)
    for (ca, aa), (cb, ab) in zip(a, b):
        assert torch.equal(ca, cb) and torch.equal(aa, ab), "one seed, two results"
    assert any(x[0].shape != y[0].shape or not torch.equal(x[0], y[0]) for x, y in zip(a, c)), "another seed, the same codes"
    for (codes, att), cap, L in zip(a, caps, QUEUE_LENS):
        assert codes.shape[-1] <= cap and 1 <= att.shape[1] <= cap and att.shape[-1] == L, "a length beyond its cap"


def check_queue_errors(dev):
    """``prompt`` / ``init_state`` raise; ``rearm_rows`` off a window boundary raises; an engine without text lengths raises."""
    from lina_speech_amd.decode import DecodeEngine
    model, texts, _ = stop_case(dev)
    kw = dict(batch_size=2, max_seqlen=8, device=dev, **GREEDY)
    with pytest.raises(NotImplementedError):
        model.generate_queue(texts[:2], prompt=torch.ones(1, 1, 2, dtype=torch.long), **kw)
    with pytest.raises(NotImplementedError):
        model.generate_queue(texts[:2], init_state=model.attentive_rnn.init_state(batch_size=2), **kw)
    with pytest.raises(ValueError):
        model.generate_queue(texts[:2], batch_size=2, max_seqlen=[8], device=dev, **GREEDY)
    with torch.inference_mode():
        x = RC.ragged_texts([5, 9], 9).to(dev)
        x_enc = RC.encode_texts(model, x, [5, 9])
        eng = DecodeEngine(model, x_enc, batch_size=2, x_lens=[5, 9])
        assert eng.window > 1
        eng.begin_greedy(16, log_att=True)
        eng.rearm_rows([1], x_enc[:1], [5])                                # step 0: a boundary
        eng.greedy_step()
        with pytest.raises(RuntimeError):
            eng.rearm_rows([1], x_enc[:1], [5])
        for _ in range(eng.window - 1):
            eng.greedy_step()
        eng.rearm_rows([0, 1], x_enc, [5, 9])                              # the next boundary
        with pytest.raises(ValueError):
            eng.rearm_rows([1, 1], x_enc, [5, 9])
        uniform = DecodeEngine(model, x_enc, batch_size=2)
        with pytest.raises(NotImplementedError):
            uniform.rearm_rows([0], x_enc[:1], [5])
