"""Queue decoding: ``LinaModel.generate_queue(texts, batch_size, ...)`` refills finished decode rows from a queue of texts
(K6g ``lina_rows_rearm`` between two replays of the decode loop's graphs); every utterance equals the same text decoded alone
(tests/queue_cases.py).  Every case runs on the CPU emulator (``emu``) and, under ``-m gpu``, on the MI355X."""
import pytest
import torch

import queue_cases as QC
import ragged_cases as RC

_REARM = [(n, dtype, d, packed, flagged) for n in (1, 3, 5) for dtype in (torch.float32, torch.bfloat16) for d in (64, 1024)
          for packed in (False, True) for flagged in ("none", "some", "all")]


# ----------------------------------------------------------------------------- K6g
@pytest.mark.parametrize("n", [1, 3, 5])
def test_rows_rearm_emu(emu, n):
    for case in _REARM:
        if case[0] == n:
            QC.check_rows_rearm("cpu", *case)


def test_rows_rearm_argument_errors_emu(emu):
    QC.check_rows_rearm_errors("cpu")


@pytest.mark.gpu
def test_rows_rearm_gpu(hip):
    for case in _REARM:
        QC.check_rows_rearm("cuda", *case)
    QC.check_rows_rearm_errors("cuda")


# ----------------------------------------------------------------------------- model, CPU (emulator)
@pytest.mark.parametrize("every", [4, 8, 16])
@pytest.mark.parametrize("B", [4, 3])
def test_queue_stops_equal_alone_emu(emu, B, every):
    QC.check_queue_stops("cpu", B, every)


def test_queue_caps_and_ring_emu(emu):
    QC.check_queue_caps("cpu")


def test_queue_invariance_and_edge_counts_emu(emu):
    QC.check_queue_invariance("cpu")


def test_queue_sampled_emu(emu):
    QC.check_queue_sampled("cpu")


def test_queue_errors_emu(emu):
    QC.check_queue_errors("cpu")


# ----------------------------------------------------------------------------- model, GPU
@pytest.mark.gpu
@pytest.mark.parametrize("every", [8, 16])
@pytest.mark.parametrize("B", [4, 3])
def test_queue_stops_equal_alone_gpu(hip, B, every):
    QC.check_queue_stops("cuda", B, every)


@pytest.mark.gpu
def test_queue_caps_and_ring_gpu(hip):
    QC.check_queue_caps("cuda")


@pytest.mark.gpu
def test_queue_invariance_sampled_errors_gpu(hip):
    QC.check_queue_invariance("cuda")
    QC.check_queue_sampled("cuda")
    QC.check_queue_errors("cuda")


@pytest.mark.gpu
def test_queue_l169_fp32_gpu(hip):
    """The L169 two-layer slice in fp32 (peaked logits: it never stops), B = 64 rows, a queue of 160 texts with step caps in
    [3, 40]: utterances 0, 63, 64, 100 and 159 equal their alone runs (codes exactly, attention within the 1e-4 of
    test_ragged_l169_fp32_gpu)."""
    from lina_speech_amd.configs import l169
    from model_cases import peak_logits
    torch.manual_seed(0)
    model = l169(n_layer=2, txt_layers=2)
    peak_logits(model)
    model = model.to("cuda", torch.float32).eval()
    N, Tmax = 160, 64
    lens = [1 + (i * 37) % Tmax for i in range(N)]
    caps = [3 + (i * 11) % 38 for i in range(N)]
    x = RC.ragged_texts(lens, Tmax, seed=23).to("cuda")
    texts = [x[i, :L] for i, L in enumerate(lens)]
    got = model.generate_queue(texts, batch_size=64, max_seqlen=caps, device="cuda", **QC.GREEDY)
    ids = [0, 63, 64, 100, 159]
    alone = [model.generate_batch(texts[i], batch_size=1, max_seqlen=caps[i], device="cuda", **QC.GREEDY) for i in ids]
    QC.assert_equals_alone([got[i] for i in ids], alone, 1e-4, "L169 fp32 queue", ids=ids)


@pytest.mark.gpu
def test_queue_b512_gpu(hip):
    """The tiny model at B = 512, a queue of 1100 texts: a handful of utterances equal the per-token module path (oracle-free:
    the same model's unfused step), as test_ragged_b512_two_engines_gpu checks its rows."""
    model = RC.tiny_model("cuda")
    N, Tmax = 1100, 64
    lens = [1 + (i * 13) % Tmax for i in range(N)]
    caps = [3 + (i * 7) % 30 for i in range(N)]
    x = RC.ragged_texts(lens, Tmax, seed=7).to("cuda")
    texts = [x[i, :L] for i, L in enumerate(lens)]
    got = model.generate_queue(texts, batch_size=512, max_seqlen=caps, device="cuda", **QC.GREEDY)
    assert len(got) == N and all(g is not None for g in got)
    ids = [0, 511, 512, 777, 1099]
    ref = [model.generate_batch(texts[i], batch_size=1, max_seqlen=caps[i], device="cuda", engine="module", **QC.GREEDY)
           for i in ids]
    QC.assert_equals_alone([got[i] for i in ids], ref, 1e-4, "B = 512 queue vs module path", ids=ids)
