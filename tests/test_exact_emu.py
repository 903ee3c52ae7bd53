"""Exact-integer checks (tests/exact_cases.py) of the kernel SOURCES on the wave64 emulator, and the one test of the method
itself.  The emulator is slow: T <= 70 and one batch row where a case would otherwise take long; tests/test_exact_gpu.py
runs the full list on the device."""
import pytest
import torch

import exact_cases as X
from kernel_cases import assert_close
from lina_speech_amd import ops

DEV = "cpu"
BF16, F32 = torch.bfloat16, torch.float32


def _projection(M, N, K, g):
    a = (torch.randn(M, K, generator=g) * 1.5).to(BF16)             # as kernel_cases.check_linear_skinny
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(BF16)
    return a, w, a.double() @ w.double().t()


def _without(a, w, rows, col):
    """What a kernel returns that loses the k-element ``col`` of ``rows`` (bf16 result of the otherwise exact product)."""
    bad = a.clone()
    bad[rows, col] = 0
    return (bad.double() @ w.double().t()).to(BF16)


def test_method_a_dropped_k_element_passes_the_tolerance_and_fails_the_exact_check():
    """The hole and its closure, no kernel involved, on the K = 1376 bf16 projection with randn operands as
    kernel_cases.check_linear_skinny builds it.

    Losing k-column c of ``a`` damages the result by the rank-1 matrix a[:, c] w[:, c]^T: about 0.6 % of max|ref| at a
    typical output, max|a[:, c]| max|w[:, c]| at the worst one.  ``assert_close`` looks at the worst one:
      * 5 x 20 outputs: a whole lost column is ACCEPTED at 2e-2 for the share of columns printed below; the column with the
        smallest worst case is the one shown;
      * 64 x 1024 outputs: some output always catches a large a and a large w, no whole column passes (smallest worst case
        measured: 3.0e-2) -- but the same element lost in ONE row (one lane of one fragment) is accepted.
    On ternary operands each of these damages changes every output it touches by exactly 1, and ``assert_exact`` rejects it."""
    g = torch.Generator().manual_seed(9)
    for M, N, rows in ((5, 20, slice(None)), (64, 1024, 13)):
        K = 1376
        a, w, ref = _projection(M, N, K, g)
        worst = a[rows].double().abs().reshape(-1, K).amax(0) * w.double().abs().amax(0) / ref.abs().max()
        col = int(worst.argmin())
        print(f"{M} x {N}, rows {rows}: a lost k-element costs {float(worst[col]):.2e} of max|ref| at the worst output for "
              f"column {col}, {float(worst.median()):.2e} for the median column; below 1.5e-2 for "
              f"{float((worst < 1.5e-2).double().mean()):.0%} of the columns")
        damaged = _without(a, w, rows, col)
        assert not torch.equal(damaged, ref.to(BF16))
        assert_close(damaged, ref, 2e-2, "method: damaged randn projection under the bf16 tolerance")       # accepted
        a3, w3 = (X.ternary(s, X.DENSITY, g, BF16) for s in ((M, K), (N, K)))
        ref3 = a3.double() @ w3.double().t()
        X.assert_exact_range({"a": a3.double(), "w": w3.double(), "y": ref3})
        X.assert_exact(ref3.to(BF16), ref3, "method: intact ternary projection")
        hit = (a3[rows].reshape(-1, K) != 0).any(0) & (w3 != 0).any(0)
        col3 = col if bool(hit[col]) else int(hit.nonzero()[0])        # (a column that holds a nonzero on both sides)
        with pytest.raises(AssertionError, match="elements differ from the exact result"):
            X.assert_exact(_without(a3, w3, rows, col3), ref3, "method: damaged ternary projection")


def test_method_range_precondition_rejects_what_is_not_exact():
    t = torch.tensor([1.0, 257.0], dtype=torch.float64)
    with pytest.raises(AssertionError, match="exceeds"):
        X.assert_exact_range({"t": t})
    X.assert_exact_range({"t": t}, limit=X.F32_LIMIT)
    with pytest.raises(AssertionError, match="not a multiple"):
        X.assert_exact_range({"t": t * 0.0625}, unit=0.125)
    with pytest.raises(AssertionError, match="fp64"):
        X.assert_exact_range({"t": t.float()})


# ----------------------------------------------------------------------------- K1 / K1d / K1w
@pytest.mark.parametrize("Dk,Dv,T,dtype", [(64, 64, 3, F32), (128, 64, 37, F32), (256, 256, 5, BF16)])
def test_exact_recurrent(emu, Dk, Dv, T, dtype):
    X.check_exact_recurrent(DEV, 1, 2, T, Dk, Dv, dtype)


@pytest.mark.parametrize("Dk,Dv,dtype", [(64, 64, F32), (256, 256, BF16)])
def test_exact_decode_update(emu, Dk, Dv, dtype):
    X.check_exact_decode_update(DEV, 2, 2, Dk, Dv, dtype)


@pytest.mark.parametrize("n_wg", [0, 3, 7])
@pytest.mark.parametrize("window", [8, 1])
@pytest.mark.parametrize("Dk,Dv,dtype,state_dtype", [(256, 256, BF16, F32), (256, 256, BF16, BF16), (64, 128, F32, F32)])
def test_exact_decode_window(emu, Dk, Dv, dtype, state_dtype, window, n_wg):
    X.check_exact_decode_window(DEV, 1, 2, Dk, Dv, dtype, state_dtype, window, n_wg)


@pytest.mark.parametrize("state_dtype", [F32, BF16])
@pytest.mark.parametrize("window", [8, 1])
def test_exact_decode_window_dv512(emu, window, state_dtype):
    X.check_exact_decode_window(DEV, 1, 2, 256, 512, BF16, state_dtype, window, 0)


# ----------------------------------------------------------------------------- K2
@pytest.mark.parametrize("Dk,Dv,T,dtype", [(64, 64, 37, F32), (128, 64, 20, F32), (128, 256, 50, BF16)])
def test_exact_chunk_generic_kernel(emu, Dk, Dv, T, dtype):
    X.check_exact_chunk(DEV, 1, 2, T, Dk, Dv, dtype)


@pytest.mark.parametrize("D,H,T", [(256, 1, 5), (256, 1, 32), (256, 1, 33), (256, 1, 70), (128, 2, 70), (64, 4, 65)])
def test_exact_chunk_full_head_kernel(emu, D, H, T):
    X.check_exact_chunk(DEV, 1, H, T, D, D, BF16)


def test_exact_chunk_dv512_one_launch_and_two(emu, monkeypatch):
    X.check_exact_chunk_dv512(DEV, monkeypatch, 1, 1, 40)


@pytest.mark.parametrize("T,nseg", [(70, 3), (65, 16)])
def test_exact_chunk_segment_parallel(emu, T, nseg):
    X.check_exact_chunk(DEV, 1, 1, T, 256, 256, BF16, nsegs=(1, nseg), fns=("chunk_gla",))


@pytest.mark.parametrize("Dk,Dv,T,dtype", [(64, 64, 70, F32), (256, 256, 40, BF16)])
def test_exact_chunk_simple_gla(emu, Dk, Dv, T, dtype):
    X.check_exact_chunk_simple(DEV, 1, 2 if Dk == 64 else 1, T, Dk, Dv, dtype)


# ----------------------------------------------------------------------------- K2b
@pytest.mark.parametrize("Dk,Dv,T,dtype", [(64, 64, 37, F32), (128, 256, 50, BF16)])
@pytest.mark.parametrize("state", [True, False])
def test_exact_chunk_bwd_generic_kernel(emu, Dk, Dv, T, dtype, state):
    X.check_exact_chunk_bwd(DEV, 1, 2, T, Dk, Dv, dtype, path="sweeps", with_h0=state, with_dht=state)


@pytest.mark.parametrize("D,H,T,nseg,state", [(256, 1, 40, 1, True), (256, 1, 40, 1, False), (256, 1, 70, 2, True),
                                              (128, 2, 70, 1, True), (64, 4, 70, 2, True), (64, 4, 70, 2, False)])
def test_exact_chunk_bwd_full_head_sweeps(emu, D, H, T, nseg, state):
    X.check_exact_chunk_bwd(DEV, 1, H, T, D, D, BF16, nseg=nseg, path="full", with_h0=state, with_dht=state)


def test_exact_chunk_bwd_value_column_blocks(emu):
    X.check_exact_chunk_bwd(DEV, 1, 1, 40, 256, 512, BF16, path="full")


@pytest.mark.parametrize("h0,dht", [(True, False), (False, True)])
@pytest.mark.parametrize("path", ["full", "sweeps"])
def test_exact_chunk_bwd_state_in_or_state_gradient_only(emu, path, h0, dht):
    X.check_exact_chunk_bwd(DEV, 1, 1, 40, 256, 256, BF16, nseg=1, path=path, with_h0=h0, with_dht=dht)


# ----------------------------------------------------------------------------- projections
@pytest.mark.parametrize("M,N,K,dtype,bias,resid", [(5, 20, 64, F32, False, False), (130, 100, 96, F32, True, True),
                                                    (70, 48, 1024, BF16, False, True), (64, 33, 1376, BF16, False, True),
                                                    (64, 4099, 32, BF16, False, False)])
def test_exact_linear_skinny(emu, M, N, K, dtype, bias, resid):
    X.check_exact_linear_skinny(DEV, M, N, K, dtype, bias=bias, resid=resid)


@pytest.mark.parametrize("M,N,K,dtype,bias,resid", [(64, 40, 1376, BF16, False, True), (64, 4099, 32, BF16, True, False),
                                                    (33, 300, 256, F32, True, True), (64, 64, 1024, BF16, False, False)])
def test_exact_linear_skinny_packed(emu, M, N, K, dtype, bias, resid):
    X.check_exact_linear_skinny_packed(DEV, M, N, K, dtype, bias=bias, resid=resid)


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("M,N,K,dtype,bias,resid", [(130, 70, 352, BF16, False, True), (200, 100, 80, F32, True, False)])
def test_exact_linear_tall(emu, variant, M, N, K, dtype, bias, resid):
    X.check_exact_linear_tall(DEV, M, N, K, dtype, variant, bias=bias, resid=resid)


@pytest.mark.parametrize("B,Tn,d,dtype", [(5, 100, 256, F32), (64, 20, 128, BF16)])
def test_exact_weighted_rows_add(emu, B, Tn, d, dtype):
    X.check_exact_weighted_rows_add(DEV, B, Tn, d, dtype)


# ----------------------------------------------------------------------------- sums, gathers, convolution, stacked operand
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_exact_embed_sum(emu, dtype):
    X.check_exact_embed_sum(DEV, dtype)


def test_exact_sums(emu):
    X.check_exact_sums(DEV)


@pytest.mark.parametrize("T,D,dtype,bias", [(5, 64, F32, False), (70, 64, F32, True), (70, 64, BF16, False),
                                            (130, 256, BF16, True)])
def test_exact_short_conv(emu, T, D, dtype, bias):
    X.check_exact_conv(DEV, 2, T, D, 4, dtype, use_bias=bias)


def test_exact_stacked_linear_operand(emu):
    """No autocast on the CPU: the K16 stacked operand (our kernel) in fp32, with and without the main / tail split."""
    X.check_exact_stacked_linear(DEV, (8, 8, 16, 16, 4), 24, 12, 3, 7, autocast=False, expect_split=False)
    X.check_exact_stacked_linear(DEV, (512, 512, 16), 16, 48, 1, 9, autocast=False, expect_split=True)
    X.check_exact_linear_train(DEV, 40, 24, True, autocast=False, B=2, T=10)
