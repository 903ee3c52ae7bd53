"""K1w's 64-lane sums (wave_sum4 of csrc/gla_decode_window.hip): four sums at one cross-lane latency in the addition order of
an xor butterfly.

* the helper on its own (lina_wave_sum_selftest), on the emulator and under ``-m gpu`` on the device, BITWISE against six
  explicit pairwise levels in torch -- a reference that shares no code with it -- on inputs whose sum depends on the order;
* both K1w kernels on the emulator, BITWISE against a build of the same sources with ``-DLINA_K1W_SUMS_BUTTERFLY=1`` (one
  shfl_xor butterfly per window slot under ``s <= j`` branches: the form the kernels had before);
* both kernels under ``-m gpu`` against the fp64 recurrence (the logic and the tolerances of
  kernel_cases.check_decode_window), at every window position of two windows, plain and packed og.
"""
import pytest
import torch
import torch.nn.functional as F

from kernel_cases import F64, O, assert_close
from lina_speech_amd import ops

B, H = 2, 3
BF, F32 = torch.bfloat16, torch.float32
# (Dk, Dv, activations, state): gates are fp32 throughout; a bf16 state is built for bf16 activations
CONFIGS = [(256, 256, BF, F32), (256, 256, BF, BF), (64, 64, BF, F32), (128, 64, F32, F32)]
GRIDS = (0, 1, 3, B * H + 5)        # the plain kernel; one workgroup for all heads; a tail round; more workgroups than heads
# windows 8 and 1 everywhere, 16 on the plain kernel only (all four sum groups; the persistent form serves <= 8), 4 once
CASES = [(c, w, g) for c in CONFIGS for w in (8, 1) for g in GRIDS] + [(c, 16, 0) for c in CONFIGS] + [(CONFIGS[2], 4, 3)]


def _case_id(case):
    (Dk, Dv, dtype, sdt), window, n_wg = case
    name = lambda t: "bf16" if t == BF else "fp32"
    return f"{Dk}x{Dv}-{name(dtype)}-S{name(sdt)}-w{window}-g{n_wg}"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


# ----------------------------------------------------------------------------- the helper
def _sum_inputs(n_waves=8):
    """randn * 2^U(-12, 12), mixed signs: the rounding of a partial sum depends on what was added before it."""
    g = torch.Generator().manual_seed(5)
    return (torch.randn(n_waves, 4, 64, generator=g) * torch.exp2(torch.rand(n_waves, 4, 64, generator=g) * 24 - 12)).float()


def _pairwise(x):
    """pairs, quads, eights, sixteens, halves, all: the tree of  a += shfl_xor(a, 1); ...; a += shfl_xor(a, 32)."""
    for _ in range(6):
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def _sequential(x):
    acc = x[..., 0].clone()
    for i in range(1, x.shape[-1]):
        acc = acc + x[..., i]
    return acc


def check_wave_sum(dev):
    x = _sum_inputs()
    ref = _pairwise(x)
    # a condition on the INPUTS: they tell addition orders apart (a left-to-right sum differs on most of the vectors)
    n_diff = int((_bits(_sequential(x)) != _bits(ref)).sum())
    assert n_diff > ref.numel() // 2, f"only {n_diff} of {ref.numel()} sequential sums differ from the pairwise ones"
    got = ops.wave_sum_selftest(x.to(dev))
    assert got.shape == ref.shape
    assert torch.equal(_bits(got), _bits(ref)), f"{int((_bits(got) != _bits(ref)).sum())} of {ref.numel()} sums differ in bits"


def test_wave_sum_bitwise_emu(emu):
    check_wave_sum("cpu")


@pytest.mark.gpu
def test_wave_sum_bitwise_gpu(hip):
    check_wave_sum("cuda")


# ----------------------------------------------------------------------------- the kernels, emulator: against the butterflies
def _run_window(dev, Dk, Dv, dtype, state_dtype, window, n_wg, packed=False):
    """2 * window + 1 consecutive decode steps from a random state (every position of two windows: a write-back feeds the
    reads after it); one reset gate (-20) inside a window.  Returns every step's og and the final hist_k / hist_c / hist_v / S."""
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    S = (r(B, H, Dk, Dv) * 0.5).to(state_dtype).to(dev)
    hk, hc = (torch.zeros(window, B * H, Dk, device=dev) for _ in range(2))
    hv = torch.zeros(window, B * H, Dv, device=dev)
    w = (1.0 + 0.1 * r(Dv)).to(dtype).to(dev)
    n_og = ops.packed_numel(B, H * Dv) if packed else B * H * Dv
    origin = torch.full((1,), 5, dtype=torch.int64, device=dev)
    outs = []
    for t in range(2 * window + 1):
        q, k = (r(B, H, Dk).to(dtype).to(dev) for _ in range(2))
        v, gate = (r(B, H, Dv).to(dtype).to(dev) for _ in range(2))
        gk = F.logsigmoid(r(B, H, Dk)) / 16
        if t == 3:
            gk[:, 0, ::7] = -20.0
        og = torch.zeros(n_og, dtype=dtype, device=dev)
        step = torch.full((1,), 5 + t, dtype=torch.int64, device=dev)
        ops.gla_decode_window(q, k, v, gk.to(dev), S, gate, w, og, hk, hc, hv, step, origin, window, 1e-5, og_packed=packed,
                              n_wg=n_wg)
        outs.append(og)
    return outs, hk, hc, hv, S


@pytest.fixture(scope="module")
def emu_butterfly():
    """The emulator build of the same sources with the sums as shfl_xor butterflies (built by this test, beside the default)."""
    from conftest import EmuBackend
    from emu import build_emu
    from lina_speech_amd import _lib
    lib = build_emu.build(defs=("-DLINA_K1W_SUMS_BUTTERFLY=1",), tag="k1w_butterfly", only=["gla_decode_window.hip"])
    return EmuBackend(_lib.bind(lib, hip_runtime=False))


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_kernels_bitwise_vs_butterfly_build(emu, emu_butterfly, case):
    (Dk, Dv, dtype, sdt), window, n_wg = case
    got = _run_window("cpu", Dk, Dv, dtype, sdt, window, n_wg)
    ops.set_backend(emu_butterfly)                                    # (the emu fixture restores the backend it found)
    ref = _run_window("cpu", Dk, Dv, dtype, sdt, window, n_wg)
    for t, (a, b) in enumerate(zip(ref[0], got[0])):
        assert torch.equal(_bits(a), _bits(b)), f"og differs at step {t} (window position {t % window})"
    for name, a, b in zip(("hist_k", "hist_c", "hist_v", "S"), ref[1:], got[1:]):
        assert torch.equal(_bits(a), _bits(b)), f"{name} differs"


# ----------------------------------------------------------------------------- the kernels, device: against the fp64 recurrence
def check_vs_fp64(dev, Dk, Dv, dtype, state_dtype, window, n_wg, packed):
    """kernel_cases.check_decode_window's comparison (every step's og, the state after each completed window, the flushed
    state; its tolerances) with a grid size and a packed og: NaN-filled history, reset gates inside and at the edge of a
    window."""
    g = torch.Generator().manual_seed(14)
    bf_state = state_dtype == BF
    rnd = lambda S: S.to(BF).to(F64)
    h0 = (torch.randn(B, H, Dk, Dv, generator=g) * 0.5).to(state_dtype).float()
    w = (1 + 0.1 * torch.randn(Dv, generator=g)).to(dtype).to(dev)
    S_w, S_ref = h0.clone().to(state_dtype).to(dev), h0.to(F64)
    st_tol = 8e-3 if bf_state else 1e-5            # bf16: one ulp (2^-8) where the fp32 and the fp64 value round apart
    tol = 2e-2 if dtype == BF else 2e-5
    hk, hc = (torch.full((window, B * H, Dk), float("nan"), device=dev) for _ in range(2))
    hv = torch.full((window, B * H, Dv), float("nan"), device=dev)
    step = torch.full((1,), 5, dtype=torch.int64, device=dev)
    origin = torch.full((1,), 5, dtype=torch.int64, device=dev)
    n_steps = 2 * window + 1
    for t in range(n_steps):
        q, k = (torch.randn(B, H, Dk, generator=g).to(dtype).to(dev) for _ in range(2))
        v = torch.randn(B, H, Dv, generator=g).to(dtype).to(dev)
        gk = F.logsigmoid(torch.randn(B, H, Dk, generator=g) * 2.0) / 4.0
        if t in (3, 7, 8, 12):
            gk[:, :, ::2] = -20.0
        gk = gk.to(dev)
        gate = torch.randn(B, H, Dv, generator=g).to(dtype).to(dev)
        og = torch.full((ops.packed_numel(B, H * Dv) if packed else B * H * Dv,), float("nan"), dtype=dtype, device=dev)
        ops.gla_decode_window(q, k, v, gk, S_w, gate, w, og, hk, hc, hv, step, origin, window, 1e-5, og_packed=packed,
                              n_wg=n_wg)
        step += 1
        qd, kd, vd, gd = (x.cpu().to(F64) for x in (q, k, v, gk))
        S_ref = S_ref * gd.exp().unsqueeze(-1) + kd.unsqueeze(-1) * vd.unsqueeze(-2)
        o_ref = torch.einsum("bhk,bhkv->bhv", qd * Dk ** -0.5, S_ref)
        og_ref = O.rmsnorm_swish_gate(o_ref, gate.cpu().to(F64), w.cpu().to(F64), 1e-5)
        og = ops.unpack_rows(og, B, H * Dv) if packed else og
        assert_close(og.view(B, H, Dv), og_ref, tol, f"K1w og (step {t}, window position {t % window}, n_wg {n_wg})")
        if (t + 1) % window == 0:                 # a completed window leaves the state fully written back
            if bf_state:
                S_ref = rnd(S_ref)
            assert_close(S_w, S_ref, st_tol, f"K1w state after window (step {t}, n_wg {n_wg})")
    pending = n_steps % window
    ops.gla_decode_window_flush(S_w, hk, hc, hv, pending)
    if bf_state and pending:
        S_ref = rnd(S_ref)
    assert_close(S_w, S_ref, st_tol, f"K1w flushed state (n_wg {n_wg})")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_kernels_vs_fp64_gpu(hip, case):
    (Dk, Dv, dtype, sdt), window, n_wg = case
    check_vs_fp64("cuda", Dk, Dv, dtype, sdt, window, n_wg, packed=False)


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [False, True])
def test_kernels_vs_fp64_gpu_packed_og(hip, packed):
    check_vs_fp64("cuda", 256, 256, BF, F32, 8, 3, packed)
