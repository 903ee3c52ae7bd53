"""What refilling finished rows buys, L169 bf16, B = 512, N = 2048 texts of 16-64 ids, sampled mode (k = 100, first quantizer), in
one process:
  * the stop token's head rows are scaled (bisection on the scale) until the mean utterance length of a 512-text probe falls in
    200-400 steps; the scale and the length histogram of the timed queue are recorded;
  * useful tokens/s = sum of utterance lengths / wall time of ``generate_queue`` against N / B back-to-back ``generate_batch``
    calls (one engine) on the same texts, three alternating repetitions; the queue stands if it wins all three;
  * ms per step of the queue loop (wall time / steps the loop ran, text encode, harvest and K6g included) against the plain loop
    of ``generate_batch`` (wall time / steps).
Prints one JSON object and writes it to profiles/queue_perf.txt.
    python tools/perf_queue.py [N] [B] [max_seqlen]"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lina_speech_amd.configs import l169  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
B = int(sys.argv[2]) if len(sys.argv) > 2 else 512
CAP = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
TMAX = 64
dev = torch.device("cuda", 0)
torch.manual_seed(0)
m = l169().eval().to(dev, torch.bfloat16)
g = torch.Generator().manual_seed(99)
lens = torch.randint(16, TMAX + 1, (N,), generator=g).tolist()
texts = [torch.randint(3, 256, (L,), generator=g).to(dev) for L in lens]
SAMPLED = dict(k=100, first_greedy_quant=1, temp=1.0, device=dev)
w0 = m.logits_head.weight.detach().clone()


def set_scale(s):
    with torch.no_grad():
        m.logits_head.weight.copy_(w0)
        m.logits_head.weight[:, 2] *= s                      # the stop token's row of every quantizer's head
    m.clear_decode_cache()


def batch_run(ids, seed):
    """One generate_batch call on the texts ``ids`` (ragged, one engine): (utterance lengths, steps the loop ran, seconds)."""
    x = torch.nn.utils.rnn.pad_sequence([texts[i] for i in ids], batch_first=True)
    x = torch.nn.functional.pad(x, (0, TMAX - x.shape[1]))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    qs, _, _, cuts = m.generate_batch(x, batch_size=len(ids), max_seqlen=CAP, x_lens=[lens[i] for i in ids], seed=seed,
                                      n_engines=1, **SAMPLED)
    torch.cuda.synchronize()
    return [int(c[1].shape[1]) for c in cuts], int(qs.shape[-1]), time.perf_counter() - t0


def mean_len(s):
    set_scale(s)
    n, _, _ = batch_run(list(range(B)), 1)
    return sum(n) / len(n)


lo, hi, scale = 1.0, 64.0, None
probes = []
for _ in range(10):                                          # a larger scale stops sooner
    mid = (lo * hi) ** 0.5
    ml = mean_len(mid)
    probes.append((round(mid, 3), round(ml, 1)))
    if 200 <= ml <= 400:
        scale = mid
        break
    lo, hi = (mid, hi) if ml > 400 else (lo, mid)
out = {"config": f"L169 bf16, B {B}, N {N} texts of 16-{TMAX} ids, sampled k=100 first quantizer, max_seqlen {CAP}",
       "scale_probes": probes, "stop_scale": scale}
if scale is None:
    out["error"] = "no stop scale gave a mean length in 200-400 steps"
else:
    set_scale(scale)
    m.generate_queue(texts[:B + 8], batch_size=B, max_seqlen=64, seed=3, max_text_len=TMAX, **SAMPLED)     # engines, graphs
    batch_run(list(range(B)), 3)
    reps = []
    for r in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = m.generate_queue(texts, batch_size=B, max_seqlen=CAP, seed=10 + r, max_text_len=TMAX, **SAMPLED)
        torch.cuda.synchronize()
        tq = time.perf_counter() - t0
        eng = next(reversed(m._decode_engines.values()))
        q_steps = eng.ring_wraps * eng.serve_cap + eng._n_done
        q_len = [int(a.shape[1]) for _, a in got]
        b_len, b_steps, tb = [], 0, 0.0
        for c in range(0, N, B):
            n, s, t = batch_run(list(range(c, min(c + B, N))), 10 + r)
            b_len += n
            b_steps += s
            tb += t
        reps.append({"queue_useful_tok_s": round(sum(q_len) / tq, 1), "batch_useful_tok_s": round(sum(b_len) / tb, 1),
                     "queue_s": round(tq, 3), "batch_s": round(tb, 3), "queue_ms_per_step": round(tq / q_steps * 1e3, 4),
                     "batch_ms_per_step": round(tb / b_steps * 1e3, 4), "queue_steps": q_steps, "batch_steps": b_steps,
                     "queue_mean_len": round(sum(q_len) / N, 1), "batch_mean_len": round(sum(b_len) / N, 1)})
    out["repetitions"] = reps
    out["queue_wins_all"] = all(r["queue_useful_tok_s"] > r["batch_useful_tok_s"] for r in reps)
    out["length_histogram_queue_last_rep"] = torch.histc(torch.tensor(q_len, dtype=torch.float32), bins=10, min=0,
                                                         max=CAP).int().tolist()
txt = json.dumps(out, indent=1)
print(txt)
with open(os.path.join(ROOT, "profiles", "queue_perf.txt"), "w") as f:
    f.write(txt + "\n")
