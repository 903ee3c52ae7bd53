"""Codec prompts of different lengths in one batch: ``generate_batch(prompt=[Q, B, P], prompt_lens=...)`` feeds every row its
own excerpt and then its own picks, each row as it decodes alone (tests/prompt_cases.py).  Every case runs on the CPU emulator
(``emu``) and, under ``-m gpu``, on the MI355X."""
import pytest
import torch

import prompt_cases as PC
import ragged_cases as RC

SAMPLED_VARIANTS = ((True, True, False), (False, False, True))     # (x_packed, loop_ctl, every length zero)
GRID = dict(B=[1, 3, 64], Q=[1, 4], d=[64, 1024], dtype=[torch.float32, torch.bfloat16])


# ----------------------------------------------------------------------------- kernel K6f
@pytest.mark.parametrize("dtype", GRID["dtype"])
@pytest.mark.parametrize("d", GRID["d"])
@pytest.mark.parametrize("Q", GRID["Q"])
@pytest.mark.parametrize("B", GRID["B"])
def test_pick_embed_forced_emu(emu, B, Q, d, dtype):
    PC.check_pick_embed_forced("cpu", B, Q, d, dtype)


@pytest.mark.parametrize("B,Q", [(3, 1), (3, 4), (64, 1)])
def test_pick_embed_forced_sampled_emu(emu, B, Q):
    PC.check_pick_embed_forced("cpu", B, Q, 64, torch.float32 if Q == 1 else torch.bfloat16, SAMPLED_VARIANTS,
                               n_sampled=1, k=10, temp=0.8, seed=11)


def test_pick_embed_forced_errors_emu(emu):
    PC.check_pick_embed_forced_errors("cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", GRID["dtype"])
@pytest.mark.parametrize("d", GRID["d"])
@pytest.mark.parametrize("Q", GRID["Q"])
@pytest.mark.parametrize("B", GRID["B"] + [512])
def test_pick_embed_forced_gpu(hip, B, Q, d, dtype):
    PC.check_pick_embed_forced("cuda", B, Q, d, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("Q", GRID["Q"])
@pytest.mark.parametrize("B", [3, 64, 512])
def test_pick_embed_forced_sampled_gpu(hip, B, Q):
    PC.check_pick_embed_forced("cuda", B, Q, 1024, torch.bfloat16, SAMPLED_VARIANTS, n_sampled=1, k=10, temp=0.8, seed=11)
    PC.check_pick_embed_forced("cuda", B, Q, 64, torch.float32, SAMPLED_VARIANTS, n_sampled=1, k=10, temp=0.8, seed=11)


@pytest.mark.gpu
def test_pick_embed_forced_errors_gpu(hip):
    PC.check_pick_embed_forced_errors("cuda")


# ----------------------------------------------------------------------------- engine
def test_forced_engine_loop_emu(emu):
    PC.check_forced_engine("cpu")


@pytest.mark.gpu
def test_forced_engine_loop_gpu(hip):
    PC.check_forced_engine("cuda")


# ----------------------------------------------------------------------------- model, CPU (emulator)
@pytest.mark.parametrize("engine", [None, "fused", "module"])
def test_prompt_rows_equal_alone_emu(emu, engine):
    PC.check_prompt_rows_alone("cpu", engine)


def test_prompt_list_form_emu(emu):
    PC.check_prompt_list_form("cpu")


def test_prompt_with_init_state_emu(emu):
    PC.check_prompt_init_state("cpu")


def test_prompt_pad_contents_do_not_matter_emu(emu):
    PC.check_prompt_pad_invariance("cpu")


def test_prompt_equal_lengths_emu(emu):
    PC.check_prompt_equal_lengths("cpu")


def test_prompt_stop_steps_emu(emu):
    PC.check_prompt_stops("cpu")


def test_prompt_argument_errors_emu(emu):
    PC.check_prompt_errors("cpu")


# ----------------------------------------------------------------------------- model, GPU
@pytest.mark.gpu
@pytest.mark.parametrize("engine", [None, "fused", "module"])
def test_prompt_rows_equal_alone_gpu(hip, engine):
    PC.check_prompt_rows_alone("cuda", engine)


@pytest.mark.gpu
def test_prompt_forms_and_state_gpu(hip):
    PC.check_prompt_list_form("cuda")
    PC.check_prompt_init_state("cuda")
    PC.check_prompt_pad_invariance("cuda")
    PC.check_prompt_errors("cuda")


@pytest.mark.gpu
def test_prompt_stop_steps_gpu(hip):
    PC.check_prompt_stops("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("B", [4, 64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_prompt_equal_lengths_gpu(hip, dtype, B):
    PC.check_prompt_equal_lengths("cuda", dtype, B)


@pytest.mark.gpu
def test_prompt_l169_fp32_gpu(hip):
    """L169-width slice, fp32, peaked logits: B = 64 ragged texts (lengths over [1, 64]) with prompt lengths (i * 7) % 25 of a
    [Q, 64, 24] prompt, max_seqlen = 40; rows (0, 5, 17, 40, 63) decoded alone with their own excerpt give the same tokens,
    stop flags and cuts, attention rows within fp32 noise of two different paths (1e-4)."""
    from lina_speech_amd.configs import l169
    from model_cases import peak_logits
    torch.manual_seed(0)
    model = l169(n_layer=2, txt_layers=2)
    peak_logits(model)
    model = model.to("cuda", torch.float32).eval()
    B, Tmax, Pn = 64, 64, 24
    lens = [1 + (i * 37) % Tmax for i in range(B)]
    lens[5] = Tmax
    plens = [(i * 7) % 25 for i in range(B)]
    x = RC.ragged_texts(lens, Tmax, seed=21).to("cuda")
    prompt = PC.prompt_tokens(model.n_quant, B, Pn, seed=23).to("cuda")
    kw = dict(max_seqlen=40, k=1, first_greedy_quant=0, device="cuda", force_max_seqlen=True)
    got = model.generate_batch(x, batch_size=B, x_lens=lens, prompt=prompt, prompt_lens=plens, **kw)
    rows = [0, 5, 17, 40, 63]
    alone = [model.generate_batch(x[i:i + 1, :lens[i]], batch_size=1,
                                  prompt=prompt[:, i:i + 1, :plens[i]] if plens[i] else None, **kw) for i in rows]
    RC.assert_rows_alone((got[0][:, rows], got[1][rows], got[2][rows], [got[3][i] for i in rows]), alone,
                         [lens[i] for i in rows], 1e-4, "L169 fp32, ragged prompts")
