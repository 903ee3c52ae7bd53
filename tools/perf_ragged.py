"""Ragged against uniform texts, L169 bf16, Tmax = 64 (as tools/perf_generate_batch.py), B = 64 and 512 in one process:
ms per token of the bare device loop (att log on, GRAPH_STEPS replays) and of generate_batch end to end (force_max_seqlen),
the two kinds alternated over repeats; prints the median and the spread (min-max) of every figure as one JSON object.
Ragged lengths are spread over [16, 64].
    python tools/perf_ragged.py [repeats] [steps]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lina_speech_amd.configs import l169  # noqa: E402
from lina_speech_amd.decode import DecodeEngine, DecodeEngineGroup  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 256
TMAX = 64
dev = torch.device("cuda", 0)
torch.manual_seed(0)
m = l169().eval().to(dev, torch.bfloat16)


def loop_ms(eng, n):
    eng.begin_greedy(n + 64, log_att=True)
    eng.greedy_steps(64)                                      # warm: graphs captured, caches settled
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.greedy_steps(n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def gen_ms(x, B, lens, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.generate_batch(x, batch_size=B, max_seqlen=n, k=1, first_greedy_quant=0, device=dev, force_max_seqlen=True,
                     x_lens=lens)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


out = {"config": f"L169 bf16, Tmax {TMAX}, ragged lengths over [16, {TMAX}], {STEPS} steps, {REPS} repeats (alternated)"}
for B in (64, 512):
    g = torch.Generator().manual_seed(1234 + B)
    x = torch.randint(3, 256, (B, TMAX), generator=g).to(dev)
    lens = torch.randint(16, TMAX + 1, (B,), generator=g)
    xr = x.clone()
    for i, L in enumerate(lens.tolist()):
        xr[i, L:] = 0
    n_eng = 2 if B >= m.AUTO_TWO_ENGINES_ROWS else 1
    with torch.inference_mode():
        live = torch.arange(TMAX, device=dev)[None, :] < lens.to(dev)[:, None]
        enc_u = m.txt_encoder(m.txt_embed(x))
        enc_r = m.txt_encoder(m.txt_embed(xr), mask=live[:, None, :] & live[:, :, None])
        mk = (lambda enc, xl: DecodeEngineGroup(m, enc, batch_size=B, n_engines=2, x_lens=xl)) if n_eng > 1 else \
            (lambda enc, xl: DecodeEngine(m, enc, batch_size=B, x_lens=xl))
        res = {"uniform_loop": [], "ragged_loop": [], "uniform_generate_batch": [], "ragged_generate_batch": []}
        engs = {"uniform": mk(enc_u, None), "ragged": mk(enc_r, lens)}
        for r in range(REPS):                                 # the bare loops alternated
            for kind, eng in engs.items():
                res[f"{kind}_loop"].append(loop_ms(eng, STEPS))
        for eng in engs.values():
            eng.close()
        del engs
        torch.cuda.empty_cache()
        gen_ms(x, B, None, 16)                                # (engines built and captured outside the timing)
        gen_ms(xr, B, lens, 16)
        for r in range(REPS):                                 # generate_batch: uniform and ragged alternated
            res["uniform_generate_batch"].append(gen_ms(x, B, None, STEPS))
            res["ragged_generate_batch"].append(gen_ms(xr, B, lens, STEPS))
        m.clear_decode_cache()
    fig = {k: {"median_ms_per_token": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
           for k, v in res.items()}
    for what in ("loop", "generate_batch"):
        u, r = fig[f"uniform_{what}"]["median_ms_per_token"], fig[f"ragged_{what}"]["median_ms_per_token"]
        fig[f"ragged_vs_uniform_{what}"] = round(r / u - 1.0, 4)
    fig["mean_len"] = float(lens.float().mean())
    out[f"B{B}"] = fig
print(json.dumps(out, indent=1))
