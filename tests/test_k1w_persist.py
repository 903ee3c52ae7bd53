"""The persistent K1w (lina_gla_decode_window_persist) against the one-workgroup-per-head kernel (lina_gla_decode_window_s):
same arithmetic in the same order, so every output is compared BITWISE -- on the CPU emulator and, under ``-m gpu``, on the
device; there also the decode engines with the persistent form against ``k1w_persist_wg = 0``."""
import pytest
import torch

from lina_speech_amd import ops


def _run_window(dev, B, H, Dk, Dv, dtype, state_dtype, window, packed, n_wg, n_steps, seed=0):
    """``n_steps`` consecutive decode steps from a random state; returns every step's og and the final hist_* / S."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    S = (r(B, H, Dk, Dv) * 0.5).to(state_dtype).to(dev)
    hk, hc = (torch.zeros(window, B * H, Dk, device=dev) for _ in range(2))
    hv = torch.zeros(window, B * H, Dv, device=dev)
    w = (1.0 + 0.1 * r(Dv)).to(dtype).to(dev)
    n_og = ops.packed_numel(B, H * Dv) if packed else B * H * Dv
    origin = torch.full((1,), 5, dtype=torch.int64, device=dev)
    outs = []
    for t in range(n_steps):
        q, k = (r(B, H, Dk).to(dtype).to(dev) for _ in range(2))
        v, gate = (r(B, H, Dv).to(dtype).to(dev) for _ in range(2))
        gk = torch.nn.functional.logsigmoid(r(B, H, Dk)) / 16
        if t == 3:
            gk[:, 0, ::7] = -20.0                                     # reset gates inside a window
        gk = gk.to(dev)                                               # fp32 gates with either activation dtype
        og = torch.zeros(n_og, dtype=dtype, device=dev)
        step = torch.full((1,), 5 + t, dtype=torch.int64, device=dev)
        ops.gla_decode_window(q, k, v, gk, S, gate, w, og, hk, hc, hv, step, origin, window, 1e-5, og_packed=packed,
                              n_wg=n_wg)
        outs.append(og)
    return outs, hk, hc, hv, S


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def check_persist_equals_plain(dev, B, H, Dk, Dv, dtype, state_dtype, window, packed, grids=None):
    """All positions of two consecutive windows (a write-back feeds later reads), for every grid size: fewer workgroups than
    heads with a tail round, one head each, more workgroups than heads."""
    BH = B * H
    n_steps = 2 * window + 1 if window > 1 else 3
    ref = _run_window(dev, B, H, Dk, Dv, dtype, state_dtype, window, packed, 0, n_steps)
    for n_wg in grids or (1, 3, BH - 1, BH, BH + 5):
        got = _run_window(dev, B, H, Dk, Dv, dtype, state_dtype, window, packed, n_wg, n_steps)
        for t, (a, b) in enumerate(zip(ref[0], got[0])):
            assert torch.equal(_bits(a), _bits(b)), f"og differs at step {t} (n_wg={n_wg})"
        for name, a, b in zip(("hist_k", "hist_c", "hist_v", "S"), ref[1:], got[1:]):
            assert torch.equal(_bits(a), _bits(b)), f"{name} differs (n_wg={n_wg})"


# Dk = 256 is built for bf16 activations (1024 threads: 128 registers each); Dk = 64 for both
CASES = [(256, 256, torch.bfloat16), (256, 128, torch.bfloat16), (64, 64, torch.bfloat16), (64, 128, torch.float32),
         (64, 256, torch.bfloat16), (128, 64, torch.float32)]


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("window", [8, 1])
@pytest.mark.parametrize("Dk,Dv,dtype", CASES)
def test_persist_bitwise_fp32_state(emu, Dk, Dv, dtype, window, packed):
    check_persist_equals_plain("cpu", 2, 3, Dk, Dv, dtype, torch.float32, window, packed)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("window", [8, 1])
@pytest.mark.parametrize("Dk,Dv", [(256, 256), (64, 64), (64, 256)])
def test_persist_bitwise_bf16_state(emu, Dk, Dv, window, packed):
    check_persist_equals_plain("cpu", 2, 3, Dk, Dv, torch.bfloat16, torch.bfloat16, window, packed)


def test_persist_rejects_what_it_does_not_serve(emu):
    def call(**kw):
        a = dict(B=1, H=2, Dk=64, Dv=64, dtype=torch.bfloat16, state_dtype=torch.float32, window=8, packed=False, n_wg=2)
        a.update(kw)
        _run_window("cpu", a["B"], a["H"], a["Dk"], a["Dv"], a["dtype"], a["state_dtype"], a["window"], a["packed"],
                    a["n_wg"], 1)
    call()
    for bad in (dict(n_wg=-1), dict(window=16), dict(Dk=256, dtype=torch.float32)):
        with pytest.raises(RuntimeError):
            call(**bad)
    with pytest.raises((RuntimeError, ValueError)):
        call(Dv=512)                                                  # (the wrapper asks for o_exchange first)


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("window", [8, 1])
@pytest.mark.parametrize("state_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Dk,Dv,dtype", CASES)
def test_persist_bitwise_gpu(hip, Dk, Dv, dtype, state_dtype, window, packed):
    if state_dtype == torch.bfloat16 and dtype != torch.bfloat16:
        dtype = torch.bfloat16                                        # a bf16 state is built for bf16 activations
    check_persist_equals_plain("cuda", 2, 3, Dk, Dv, dtype, state_dtype, window, packed)


@pytest.mark.gpu
def test_persist_bitwise_gpu_headline_shape(hip):
    """256 rows x 4 heads of 256 x 256 (one engine of the headline): grids below, at and above the chip's 256 CUs."""
    check_persist_equals_plain("cuda", 256, 4, 256, 256, torch.bfloat16, torch.float32, 8, True, grids=(128, 192, 256, 1000))


def _engine_outputs(m, x, n_engines, n, wg, **extra):
    from lina_speech_amd.decode import DecodeEngine, DecodeEngineGroup
    m.clear_decode_cache()
    ops.POLICY.k1w_persist_wg = ops.POLICY.k1w_persist_wg_group = wg
    seen, plain = [], ops.gla_decode_window

    def spy(*args, **kw):                                          # what the step really launches (capture included)
        seen.append(kw.get("n_wg", 0))
        return plain(*args, **kw)
    ops.gla_decode_window = spy
    try:
        out = m.generate_batch(x, batch_size=x.shape[0], max_seqlen=n, k=1, first_greedy_quant=0, force_max_seqlen=True,
                               device="cuda", n_engines=n_engines, **extra)
    finally:
        ops.gla_decode_window = plain
    assert seen and all(g == wg for g in seen), f"K1w launched with n_wg {sorted(set(seen))}, expected {wg}"
    eng = next(reversed(m._decode_engines.values()))
    assert isinstance(eng, DecodeEngineGroup if n_engines == 2 else DecodeEngine)
    engines = eng.engines if n_engines == 2 else [eng]
    assert all(e.k1w_persist_wg == wg for e in engines)
    with torch.inference_mode():                                   # (the engine's tensors were made in inference mode)
        states = [torch.stack([st[3] for st in e.state.states]).clone() for e in engines]   # flushed: pending steps applied
    return out, states


@pytest.mark.gpu
@pytest.mark.parametrize("n_engines,ragged", [(2, False), (1, False), (2, True)])
def test_engines_with_persistent_k1w_bit_identical(hip, n_engines, ragged):
    """DecodeEngineGroup 2 x 256 rows / DecodeEngine 512 rows (L169, bf16, peaked logits), 66 free-running steps: greedy
    tokens, stop flags, attention rows and the flushed recurrent state with the persistent K1w == with the plain kernel."""
    from lina_speech_amd.configs import l169
    from model_cases import peak_logits
    torch.manual_seed(0)
    m = peak_logits(l169().eval()).to("cuda", torch.bfloat16)
    B, n = 512, 66
    gen = torch.Generator().manual_seed(21)
    x = torch.randint(3, 256, (B, 24), generator=gen).cuda()
    extra = dict(x_lens=torch.randint(5, 25, (B,), generator=gen).tolist()) if ragged else {}
    keep = ops.POLICY.k1w_persist_wg, ops.POLICY.k1w_persist_wg_group
    try:
        ref, ref_S = _engine_outputs(m, x, n_engines, n, 0, **extra)
        for wg in (192, 256):
            got, got_S = _engine_outputs(m, x, n_engines, n, wg, **extra)
            assert torch.equal(ref[0], got[0]), f"greedy tokens differ (n_wg={wg})"
            assert torch.equal(ref[2], got[2]), f"stop flags differ (n_wg={wg})"
            assert torch.equal(_bits(ref[1]), _bits(got[1])), f"attention rows differ (n_wg={wg})"
            for a, b in zip(ref_S, got_S):
                assert torch.equal(_bits(a), _bits(b)), f"flushed state differs (n_wg={wg})"
    finally:
        ops.POLICY.k1w_persist_wg, ops.POLICY.k1w_persist_wg_group = keep
        m.clear_decode_cache()
