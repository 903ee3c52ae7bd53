"""Ragged text: ``generate_batch(x, batch_size, ..., x_lens=...)`` decodes right-padded texts of different lengths in one
batch, each row as its text alone (tests/ragged_cases.py).  Every case runs on the CPU emulator (``emu``) and, under
``-m gpu``, on the MI355X."""
import pytest
import torch

import ragged_cases as RC


# ----------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d", [64, 1024])
@pytest.mark.parametrize("B", [1, 3])
def test_ragged_cross_kernels_emu(emu, B, d, dtype):
    RC.check_ragged_kernels("cpu", B, d, dtype, shared_pe=False)
    RC.check_ragged_kernels("cpu", B, d, dtype, shared_pe=True)


def test_ragged_cross_kernels_emu_b64(emu):
    RC.check_ragged_kernels("cpu", 64, 64, torch.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d", [64, 1024])
@pytest.mark.parametrize("B", [1, 3, 64, 512])
def test_ragged_cross_kernels_gpu(hip, B, d, dtype):
    RC.check_ragged_kernels("cuda", B, d, dtype, shared_pe=False)
    RC.check_ragged_kernels("cuda", B, d, dtype, shared_pe=True)


# ----------------------------------------------------------------------------- model, CPU (emulator)
def test_ragged_generate_rows_equal_alone_emu(emu):
    RC.check_ragged_generate("cpu")


def test_ragged_generate_stop_steps_emu(emu):
    RC.check_ragged_stops("cpu")


def test_ragged_generate_with_init_state_emu(emu):
    RC.check_ragged_init_state("cpu")


def test_ragged_pad_contents_do_not_matter_emu(emu):
    RC.check_ragged_pad_invariance("cpu")


def test_ragged_argument_errors_emu(emu):
    RC.check_ragged_errors("cpu")


def test_ragged_engine_teacher_forced_emu(emu):
    model = RC.tiny_model("cpu")
    lens = list(RC.RAGGED_LENS)
    x = RC.ragged_texts(lens, 64)
    RC.check_ragged_teacher_forced("cpu", model, x, lens, range(4), 6, 1e-5)


# ----------------------------------------------------------------------------- model, GPU
@pytest.mark.gpu
def test_ragged_generate_rows_equal_alone_gpu(hip):
    RC.check_ragged_generate("cuda")
    RC.check_ragged_stops("cuda")
    RC.check_ragged_init_state("cuda")
    RC.check_ragged_pad_invariance("cuda")
    RC.check_ragged_errors("cuda")


def _l169_slice(dtype):
    from lina_speech_amd.configs import l169
    from model_cases import peak_logits
    torch.manual_seed(0)
    model = l169(n_layer=2, txt_layers=2)
    peak_logits(model)
    return model.to("cuda", dtype).eval()


@pytest.mark.gpu
def test_ragged_l169_fp32_gpu(hip):
    """L169-width slice, fp32, peaked logits: B = 64 ragged texts (lengths over [1, 64]); a subset of rows decoded alone gives
    the same tokens and stop steps, attention rows within fp32 noise; logits per step within fp32 noise (teacher-forced)."""
    model = _l169_slice(torch.float32)
    B, Tmax = 64, 64
    lens = [1 + (i * 37) % Tmax for i in range(B)]
    lens[5] = Tmax
    x = RC.ragged_texts(lens, Tmax, seed=21).to("cuda")
    kw = dict(max_seqlen=24, k=1, first_greedy_quant=0, device="cuda", force_max_seqlen=True)
    got = model.generate_batch(x, batch_size=B, x_lens=lens, **kw)
    rows = [0, 5, 17, 40, 63]
    alone = [model.generate_batch(x[i:i + 1, :lens[i]], batch_size=1, **kw) for i in rows]
    RC.assert_rows_alone((got[0][:, rows], got[1][rows], got[2][rows], [got[3][i] for i in rows]), alone,
                         [lens[i] for i in rows], 1e-4, "L169 fp32")
    RC.check_ragged_teacher_forced("cuda", model, x, lens, rows, 8, 1e-4)


@pytest.mark.gpu
def test_ragged_l169_bf16_teacher_forced_gpu(hip):
    """The same slice in bf16: teacher-forced (the ragged engine's greedy picks fed to both sides, so that one near-tie
    cannot fork the sequences); logits within the bf16 bound of the L169 bf16 engine check, picks equal away from near-ties."""
    model = _l169_slice(torch.bfloat16)
    B, Tmax = 64, 64
    lens = [1 + (i * 29) % Tmax for i in range(B)]
    x = RC.ragged_texts(lens, Tmax, seed=22).to("cuda")
    RC.check_ragged_teacher_forced("cuda", model, x, lens, [0, 3, 31, 62], 12, 1e-2)


@pytest.mark.gpu
def test_ragged_b512_two_engines_gpu(hip):
    """B = 512 on the default two-engine path: pad contents do not matter; a few rows equal the per-token module path
    (oracle-free: the same model's unfused step) in tokens."""
    from lina_speech_amd.decode import DecodeEngineGroup
    model = RC.tiny_model("cuda")
    B, Tmax = 512, 64
    lens = [1 + (i * 13) % Tmax for i in range(B)]
    xa = RC.ragged_texts(lens, Tmax, seed=6, pad=0).to("cuda")
    xb = RC.ragged_texts(lens, Tmax, seed=6, pad="random").to("cuda")
    kw = dict(max_seqlen=16, k=1, first_greedy_quant=0, device="cuda", force_max_seqlen=True)
    a = model.generate_batch(xa, batch_size=B, x_lens=lens, **kw)
    assert isinstance(next(reversed(model._decode_engines.values())), DecodeEngineGroup)
    b = model.generate_batch(xb, batch_size=B, x_lens=lens, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "pad contents changed the decode at B = 512"
    for i in (0, 255, 256, 511):
        L = lens[i]
        m = model.generate_batch(xa[i:i + 1], batch_size=1, x_lens=[L], engine="module", **kw) if L < Tmax else \
            model.generate_batch(xa[i:i + 1], batch_size=1, engine="module", **kw)
        assert torch.equal(a[0][:, i], m[0][:, 0]), f"row {i} (L = {L}): tokens differ from the module path"
        err = float((a[1][i].float() - m[1][0].float()).abs().max() / m[1][0].float().abs().max())
        assert err < 1e-4, f"row {i}: attention log differs from the module path by {err:.2e}"
