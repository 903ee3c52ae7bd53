"""The ragged vocoder on the MI355X (tests/vocoder_ragged_cases.py): the cases of test_vocoder_ragged_emu.py on the device,
and one row of the full-size decoder against the fp64 oracle."""
import pytest

import vocoder_ragged_cases as VC

DEV = "cuda"
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("C,dtype,ada", VC.K8R_CASES, ids=["C64-f32", "C96-bf16-ada"])
def test_dwconv7_ln_ragged(hip, monkeypatch, C, dtype, ada):
    VC.run_guarded(lambda: VC.check_dwconv7_ln_ragged(DEV, C, dtype, ada), VC.K8R_N_CASE, VC.K8R_N_LIB, DEV, monkeypatch)


@pytest.mark.parametrize("shape,lens", VC.K9R_CASES, ids=["T6-win40", "T20-win64"])
def test_istft_ola_ragged(hip, monkeypatch, shape, lens):
    VC.run_guarded(lambda: VC.check_istft_ola_ragged(DEV, shape, lens), VC.K9R_N_CASE, VC.K9R_N_LIB, DEV, monkeypatch)


@pytest.mark.parametrize("act", [None, "silu"], ids=["plain", "silu"])
@pytest.mark.parametrize("shape,lens,dtype", VC.K10G_CASES, ids=["C64-f32", "C96-bf16", "C768-L300-f32"])
def test_group_norm_ragged(hip, monkeypatch, shape, lens, dtype, act):
    n_case, n_lib = VC.k10g_counts(shape[0])
    VC.run_guarded(lambda: VC.check_group_norm_ragged(DEV, shape, lens, dtype, act), n_case, n_lib, DEV, monkeypatch)


def test_kernel_argument_errors(hip):
    VC.check_kernel_argument_errors(DEV)


def test_module_rows_equal_alone(hip):
    VC.check_module_rows(DEV)


def test_module_pads_uniform_and_list_form(hip):
    VC.check_module_pads_uniform_list(DEV)


def test_module_errors(hip):
    VC.check_module_errors(DEV)


def test_full_size_row_matches_cpu_oracle(hip):
    VC.check_full_size_row(DEV)


def test_synthesize_equals_alone_and_empty_cuts(hip):
    VC.check_synthesize_equals_alone(DEV)


def test_synthesize_vocoder_batch(hip):
    VC.check_synthesize_vocoder_batch(DEV)


def test_synthesize_errors(hip):
    VC.check_synthesize_errors(DEV)
