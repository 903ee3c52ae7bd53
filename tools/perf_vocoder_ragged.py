"""What the ragged vocoder costs: the full-size WavTokenizer decoder (dim 768, 12 ConvNeXt blocks, n_fft 1280,
hop 320), B = 64 utterances of 200..750 frames (uniform, one of them 750), fp32 and bf16, in one process:
  (a) the ragged call           voc(codes [1, 64, 750], lens=...);
  (b) 64 alone calls            voc(codes[:, b:b+1, :L_b]) -- the only correct way without ``lens``;
  (c) the uniform call          voc(codes [1, 64, 750]) -- wrong audio for the 63 shorter rows, the cost floor of the padded shape;
and K10g by itself on the [64, 768, 750] activations of ``pos_net`` with the same lengths: time per launch and achieved bytes/s
against the bytes it must move, 2 * B * C * mean(L) * e (one read, one write of the live elements), next to ``F.group_norm`` on
the same padded block.  Every shape is warmed up first; times are device events around ``reps`` back-to-back calls, three
alternating repetitions of (a), (c), (b), the median reported.  Prints one JSON object per dtype (as soon as it is measured) and
writes them to profiles/vocoder_ragged_perf.txt.
    python tools/perf_vocoder_ragged.py [B] [reps]"""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lina_speech_amd import ops  # noqa: E402
from lina_speech_amd.vocoder import WavTokenizerDecoder  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
LMIN, LMAX = 200, 750
assert torch.cuda.is_available(), "perf_vocoder_ragged.py measures on the GPU: there is no CPU fallback"
dev = torch.device("cuda", 0)


def timed(fn, reps):
    """ms per call: device events around ``reps`` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def measure(dtype):
    torch.manual_seed(0)
    voc = WavTokenizerDecoder().eval().to(dev, dtype)
    voc.head.istft.window = torch.hann_window(voc.head.istft.win_length, device=dev)     # the ISTFT stays in fp32
    g = torch.Generator().manual_seed(7)
    lens = torch.randint(LMIN, LMAX + 1, (B,), generator=g).tolist()
    lens[0] = LMAX
    codes = torch.randint(0, 4096, (1, B, LMAX), generator=g).to(dev)
    bw = torch.tensor([0], device=dev)
    rows = [codes[:, b:b + 1, :L].contiguous() for b, L in enumerate(lens)]
    ragged = lambda: voc(codes, bandwidth_id=bw, lens=lens)
    uniform = lambda: voc(codes, bandwidth_id=bw)

    def alone():
        for r in rows:
            voc(r, bandwidth_id=bw)

    for fn in (ragged, uniform, alone):                      # every shape once: code objects, library algorithm choices
        fn()
    ragged(), uniform()
    t = {"a": [], "b": [], "c": []}
    for _ in range(3):
        t["a"].append(timed(ragged, REPS))
        t["c"].append(timed(uniform, REPS))
        t["b"].append(timed(alone, 1))
    # K10g alone
    e = torch.empty(0, dtype=dtype).element_size()
    C, G = 768, 32
    x = torch.randn(B, C, LMAX, device=dev).to(dtype)
    w, bias = torch.ones(C, device=dev, dtype=dtype), torch.zeros(C, device=dev, dtype=dtype)
    ld = torch.tensor(lens, dtype=torch.int32, device=dev)
    k10g = lambda: ops.group_norm_ragged(x, G, w, bias, 1e-6, "silu", ld)
    lib = lambda: F.silu(F.group_norm(x, G, w, bias, 1e-6))
    k10g(), lib()
    tk = statistics.median(timed(k10g, 20) for _ in range(3))
    tl = statistics.median(timed(lib, 20) for _ in range(3))
    need = 2 * B * C * (sum(lens) / B) * e
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"config": f"WavTokenizer decoder, {str(dtype)[6:]}, B {B}, frames uniform in {LMIN}..{LMAX} (mean {sum(lens) / B:.0f})",
            "a_ragged_ms": round(med["a"], 3), "b_alone_calls_ms": round(med["b"], 3), "c_uniform_padded_ms": round(med["c"], 3),
            "a_over_c": round(med["a"] / med["c"], 3), "b_over_a": round(med["b"] / med["a"], 2),
            "all_repetitions_ms": {k: [round(x, 3) for x in v] for k, v in t.items()},
            "k10g_silu_ms": round(tk, 4), "k10g_needed_bytes": int(need), "k10g_achieved_GB_s": round(need / tk / 1e6, 1),
            "library_group_norm_silu_padded_ms": round(tl, 4), "k10g_launches_per_call": 10}


out = []
for dtype in (torch.float32, torch.bfloat16):
    out.append(measure(dtype))
    print(json.dumps(out[-1]), flush=True)
    with open(os.path.join(ROOT, "profiles", "vocoder_ragged_perf.txt"), "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
