"""Exact-integer checks (tests/exact_cases.py) on the device: the full list of kernels, variants and shapes -- the bf16-only
paths (MFMA 16x16x32 fragment layouts, full-head K2 / K2b with 1 / 2 / 4 heads per workgroup, NCB = 2, segment-parallel
form, Dk = 256 K1w and its persistent form, fragment-major and tall projections, the autocast training GEMMs) held to the
fp64 oracle bit for bit.  Run with ``pytest -m gpu``."""
import pytest
import torch

import exact_cases as X

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


# ----------------------------------------------------------------------------- K1 / K1d / K1w
@pytest.mark.gpu
@pytest.mark.parametrize("Dk,Dv,T,dtype", [(64, 64, 3, F32), (128, 64, 37, F32), (256, 256, 37, BF16)])
def test_exact_recurrent(hip, Dk, Dv, T, dtype):
    X.check_exact_recurrent(DEV, 2, 2, T, Dk, Dv, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("Dk,Dv,dtype", [(64, 64, F32), (256, 256, BF16)])
def test_exact_decode_update(hip, Dk, Dv, dtype):
    X.check_exact_decode_update(DEV, 5, 4, Dk, Dv, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("n_wg", [0, 3, 2 * 3 + 5])
@pytest.mark.parametrize("window", [8, 1])
@pytest.mark.parametrize("Dk,Dv,dtype,state_dtype", [(256, 256, BF16, F32), (256, 256, BF16, BF16), (64, 128, F32, F32)])
def test_exact_decode_window(hip, Dk, Dv, dtype, state_dtype, window, n_wg):
    X.check_exact_decode_window(DEV, 2, 3, Dk, Dv, dtype, state_dtype, window, n_wg)


@pytest.mark.gpu
@pytest.mark.parametrize("state_dtype", [F32, BF16])
@pytest.mark.parametrize("window", [8, 1])
def test_exact_decode_window_dv512(hip, window, state_dtype):
    # 256 x 512: the column halves meet in o_exchange; the persistent form does not serve Dv > 256
    X.check_exact_decode_window(DEV, 2, 3, 256, 512, BF16, state_dtype, window, 0)


# ----------------------------------------------------------------------------- K2
@pytest.mark.gpu
@pytest.mark.parametrize("Dk,Dv,T,dtype", [(64, 64, 37, F32), (128, 64, 20, F32), (128, 256, 50, BF16)])
def test_exact_chunk_generic_kernel(hip, Dk, Dv, T, dtype):
    X.check_exact_chunk(DEV, 2, 2, T, Dk, Dv, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("D,H,T", [(256, 4, 5), (256, 4, 32), (256, 4, 33), (256, 4, 200), (128, 2, 300), (64, 4, 257),
                                   (64, 16, 257)])
def test_exact_chunk_full_head_kernel(hip, D, H, T):
    X.check_exact_chunk(DEV, 2, H, T, D, D, BF16)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,T", [(2, 2, 100), (1, 8, 33)])          # 8 heads: the XCD-paired block-id mapping
def test_exact_chunk_dv512_one_launch_and_two(hip, monkeypatch, B, H, T):
    X.check_exact_chunk_dv512(DEV, monkeypatch, B, H, T)


# nseg = 16 at T = 257: more segments requested than 32-token chunks can fill (9 hold tokens)
@pytest.mark.gpu
@pytest.mark.parametrize("D,H,T,nseg", [(256, 2, 100, 3), (256, 2, 300, 4), (256, 2, 257, 16), (64, 4, 100, 3)])
def test_exact_chunk_segment_parallel(hip, D, H, T, nseg):
    X.check_exact_chunk(DEV, 2, H, T, D, D, BF16, nsegs=(1, nseg), fns=("chunk_gla",))


@pytest.mark.gpu
@pytest.mark.parametrize("Dk,Dv,T,dtype", [(64, 64, 70, F32), (256, 256, 256, BF16)])
def test_exact_chunk_simple_gla(hip, Dk, Dv, T, dtype):
    X.check_exact_chunk_simple(DEV, 2, 2, T, Dk, Dv, dtype)


# ----------------------------------------------------------------------------- K2b
@pytest.mark.gpu
@pytest.mark.parametrize("state", [True, False])
@pytest.mark.parametrize("Dk,Dv,T,dtype", [(64, 64, 37, F32), (128, 256, 50, BF16)])
def test_exact_chunk_bwd_generic_kernel(hip, Dk, Dv, T, dtype, state):
    X.check_exact_chunk_bwd(DEV, 2, 2, T, Dk, Dv, dtype, path="sweeps", with_h0=state, with_dht=state)


@pytest.mark.gpu
@pytest.mark.parametrize("state", [True, False])
@pytest.mark.parametrize("D,H,T,nseg", [(256, 1, 40, 1), (256, 1, 150, 1), (256, 1, 300, 4), (128, 2, 150, 1), (64, 4, 150, 2)])
def test_exact_chunk_bwd_full_head_sweeps(hip, D, H, T, nseg, state):
    X.check_exact_chunk_bwd(DEV, 2, H, T, D, D, BF16, nseg=nseg, path="full", with_h0=state, with_dht=state)


@pytest.mark.gpu
@pytest.mark.parametrize("state", [True, False])
def test_exact_chunk_bwd_value_column_blocks(hip, state):
    X.check_exact_chunk_bwd(DEV, 1, 1, 40, 256, 512, BF16, path="full", with_h0=state, with_dht=state)


@pytest.mark.gpu
@pytest.mark.parametrize("h0,dht", [(True, False), (False, True)])
@pytest.mark.parametrize("path", ["full", "sweeps"])
def test_exact_chunk_bwd_state_in_or_state_gradient_only(hip, path, h0, dht):
    X.check_exact_chunk_bwd(DEV, 2, 1, 40, 256, 256, BF16, nseg=1, path=path, with_h0=h0, with_dht=dht)


# ----------------------------------------------------------------------------- projections
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,dtype,bias,resid", [(5, 20, 64, F32, False, False), (130, 100, 96, F32, True, True),
                                                    (70, 1024, 1024, BF16, False, True), (64, 1024, 1376, BF16, False, True),
                                                    (64, 4099, 1024, BF16, False, False),
                                                    (70, 4099, 1376, BF16, True, True)])
def test_exact_linear_skinny(hip, M, N, K, dtype, bias, resid):
    X.check_exact_linear_skinny(DEV, M, N, K, dtype, bias=bias, resid=resid)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,dtype,bias,resid", [(64, 1024, 1376, BF16, False, True), (64, 4099, 1024, BF16, True, False),
                                                    (33, 300, 256, F32, True, True), (64, 64, 1024, BF16, False, False)])
def test_exact_linear_skinny_packed(hip, M, N, K, dtype, bias, resid):
    X.check_exact_linear_skinny_packed(DEV, M, N, K, dtype, bias=bias, resid=resid)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("M,N,K,dtype,bias,resid", [(130, 1024, 1376, BF16, False, True), (200, 4099, 1024, F32, True, False)])
def test_exact_linear_tall(hip, variant, M, N, K, dtype, bias, resid):
    X.check_exact_linear_tall(DEV, M, N, K, dtype, variant, bias=bias, resid=resid)


@pytest.mark.gpu
@pytest.mark.parametrize("B,Tn,d,dtype", [(5, 100, 256, F32), (64, 20, 1024, BF16)])
def test_exact_weighted_rows_add(hip, B, Tn, d, dtype):
    X.check_exact_weighted_rows_add(DEV, B, Tn, d, dtype)


# ----------------------------------------------------------------------------- sums, gathers, convolution
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_exact_embed_sum(hip, dtype):
    X.check_exact_embed_sum(DEV, dtype)


@pytest.mark.gpu
def test_exact_sums(hip):
    X.check_exact_sums(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("T,D,dtype,bias", [(5, 64, F32, False), (70, 64, F32, True), (70, 64, BF16, False),
                                            (515, 256, BF16, False), (515, 256, BF16, True)])
def test_exact_short_conv(hip, T, D, dtype, bias):
    X.check_exact_conv(DEV, 2, T, D, 4, dtype, use_bias=bias)


# ----------------------------------------------------------------------------- the autocast training GEMM path
@pytest.mark.gpu
@pytest.mark.parametrize("n_out,n_in,bias", [(1024, 1365, True), (2730, 1024, True), (1024, 1024, False), (1024, 16, True),
                                             (4112, 1024, False)])
def test_exact_linear_train_path_under_autocast(hip, n_out, n_in, bias):
    X.check_exact_linear_train(DEV, n_out, n_in, bias)                  # 300 tokens


@pytest.mark.gpu
def test_exact_stacked_linear_under_autocast(hip):
    """The L169 mixer's stack (q | k | v | g | low-rank 16 | pad 48) under autocast: the 256-aligned main + tail form of the
    GEMMs at 300 tokens; and, at a narrow input (n_in = 64, to keep the fp64 reference small), the 8192 tokens from which
    the main rows' dW is token-split as well -- every dW entry is a sum of at most 8192 products of magnitude <= 1, far
    below 2^24 (asserted)."""
    rows = (1024, 1024, 1024, 1024, 16)
    X.check_exact_stacked_linear(DEV, rows, 1024, 48, 2, 150, autocast=True, expect_split=True, expect_token_split=False)
    X.check_exact_stacked_linear(DEV, rows, 64, 48, 2, 4096, autocast=True, expect_split=True, expect_token_split=True)
    X.check_exact_stacked_linear(DEV, (8, 8, 16, 16, 4), 24, 12, 3, 7, autocast=False, expect_split=False)
