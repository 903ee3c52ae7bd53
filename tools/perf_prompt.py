"""What codec prompts of different lengths cost, L169 bf16, T_txt = 64, B = 64 and 512 (one engine: a prompt keeps one), in one
process:
  * ms per token of the bare device loop (att log on, GRAPH_STEPS replays) in its forced configuration with every
    force_len = 0 (K6f instead of K6d, nothing forced) against the unforced loop, the two alternated over repeats;
  * generate_batch end to end (force_max_seqlen) with prompt lengths spread over [p, 3p] against the uniform call with every
    prompt 3p long, alternated.
Prints the median and the spread (min-max) of every figure as one JSON object -- the spread of the unforced loop is the
session's run-to-run noise the forced figure is to be read against.
    python tools/perf_prompt.py [repeats] [steps] [p]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lina_speech_amd.configs import l169  # noqa: E402
from lina_speech_amd.decode import DecodeEngine  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 256
P = int(sys.argv[3]) if len(sys.argv) > 3 else 32
TTXT = 64
dev = torch.device("cuda", 0)
torch.manual_seed(0)
m = l169().eval().to(dev, torch.bfloat16)
Q = m.n_quant


def loop_ms(eng, n, forced):
    eng.begin_greedy(n + 64, log_att=True, forced=forced)
    eng.greedy_steps(64)                                      # warm: graphs captured, caches settled
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.greedy_steps(n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def gen_ms(x, B, prompt, lens, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.generate_batch(x, batch_size=B, max_seqlen=n, k=1, first_greedy_quant=0, device=dev, force_max_seqlen=True,
                     prompt=prompt, prompt_lens=lens, n_engines=1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


out = {"config": f"L169 bf16, T_txt {TTXT}, prompt lengths over [{P}, {3 * P}] against {3 * P}, {STEPS} steps, "
                 f"{REPS} repeats (alternated)"}
for B in (64, 512):
    g = torch.Generator().manual_seed(4321 + B)
    x = torch.randint(3, 256, (B, TTXT), generator=g).to(dev)
    prompt = torch.randint(3, 250, (Q, B, 3 * P), generator=g).to(dev)
    lens = torch.randint(P, 3 * P + 1, (B,), generator=g)
    lens[0], lens[1] = P, 3 * P
    with torch.inference_mode():
        eng = DecodeEngine(m, m.txt_encoder(m.txt_embed(x)), batch_size=B)
        nothing = (torch.zeros(Q, B, 1, dtype=torch.long, device=dev), [0] * B)
        res = {"unforced_loop": [], "forced_len0_loop": [], "uniform_3p_generate_batch": [], "ragged_generate_batch": []}
        for r in range(REPS):                                 # the bare loops alternated
            res["unforced_loop"].append(loop_ms(eng, STEPS, None))
            res["forced_len0_loop"].append(loop_ms(eng, STEPS, nothing))
        eng.close()
        del eng
        torch.cuda.empty_cache()
        gen_ms(x, B, prompt, None, 3 * P + 17)                # (engine built, both loops captured outside the timing)
        gen_ms(x, B, prompt, lens, 3 * P + 17)
        for r in range(REPS):                                 # generate_batch: uniform and ragged prompts alternated
            res["uniform_3p_generate_batch"].append(gen_ms(x, B, prompt, None, STEPS))
            res["ragged_generate_batch"].append(gen_ms(x, B, prompt, lens, STEPS))
        m.clear_decode_cache()
    unit = {"loop": "ms_per_token", "batch": "ms_per_call"}
    fig = {k: {f"median_{unit[k.rsplit('_', 1)[1]]}": round(statistics.median(v), 4), "min": round(min(v), 4),
               "max": round(max(v), 4)} for k, v in res.items()}
    fig["forced_len0_vs_unforced_loop"] = round(statistics.median(res["forced_len0_loop"])
                                                / statistics.median(res["unforced_loop"]) - 1.0, 4)
    fig["unforced_loop_spread"] = round(max(res["unforced_loop"]) / min(res["unforced_loop"]) - 1.0, 4)
    fig["ragged_vs_uniform_3p_generate_batch"] = round(statistics.median(res["ragged_generate_batch"])
                                                      / statistics.median(res["uniform_3p_generate_batch"]) - 1.0, 4)
    fig["mean_prompt_len"] = float(lens.float().mean())
    out[f"B{B}"] = fig
print(json.dumps(out, indent=1))
