"""K1w, one workgroup per head against the persistent form (lina_gla_decode_window_persist) -- ONE process, forms alternating,
several passes (profiles/k1w_persist_sweep.txt is this tool's output):

  kernel : K1w alone at L169's head shape (H = 4, 256 x 256, bf16, fp32 state, W = 8), by WINDOW POSITION (0 .. 6 read the
           state, 7 writes it back), at 64 / 256 / 512 rows; HIP events around a run of launches at one position
  loop   : the device-side greedy loop, ms per token: DecodeEngineGroup 2 x 256 and 2 x 192 rows, DecodeEngine 512 / 256 / 64

    python tools/perf_k1w_persist.py [--passes 3] [--grids 128,160,192,224,256] [--loops 2x512,1x512] [--skip-kernel] [--skip-loop]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lina_speech_amd import ops  # noqa: E402

W = 8


def settle(seconds=1.5):
    """Clocks: a second and a half of streaming before anything is timed (measuring guide: settled clocks)."""
    a = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        a.add_(1)
    torch.cuda.synchronize()


def kernel_case(rows, H=4, Dk=256, Dv=256):
    g = torch.Generator().manual_seed(rows)
    r = lambda *s: torch.randn(*s, generator=g)
    dev, bf = "cuda", torch.bfloat16
    c = dict(q=r(rows, H, Dk).to(bf).to(dev), k=r(rows, H, Dk).to(bf).to(dev), v=r(rows, H, Dv).to(bf).to(dev),
             gate=r(rows, H, Dv).to(bf).to(dev), gk=(torch.nn.functional.logsigmoid(r(rows, H, Dk)) / 16).to(dev),
             S=torch.zeros(rows, H, Dk, Dv, device=dev), w=torch.ones(Dv, dtype=bf, device=dev),
             hk=torch.zeros(W, rows * H, Dk, device=dev), hc=torch.zeros(W, rows * H, Dk, device=dev),
             hv=torch.zeros(W, rows * H, Dv, device=dev), og=torch.zeros(ops.packed_numel(rows, H * Dv), dtype=bf, device=dev),
             origin=torch.zeros(1, dtype=torch.int64, device=dev))
    c["steps"] = [torch.full((1,), j, dtype=torch.int64, device=dev) for j in range(W)]
    return c


def time_position(c, j, n_wg, reps):
    def launch():
        ops.gla_decode_window(c["q"], c["k"], c["v"], c["gk"], c["S"], c["gate"], c["w"], c["og"], c["hk"], c["hc"], c["hv"],
                              c["steps"][j], c["origin"], W, 1e-5, og_packed=True, n_wg=n_wg)
    launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def sweep_kernel(grids, passes, reps=20):
    print("== K1w alone, us per launch by window position (median of passes; position 7 = write-back)")
    for rows in (64, 256, 512):
        c = kernel_case(rows)
        res = {g: [[] for _ in range(W)] for g in grids}
        for _ in range(passes):
            for g in grids:                                          # forms alternate inside a pass
                for j in range(W):
                    res[g][j].append(time_position(c, j, g, reps))
        mb = rows * 4 * 256 * 256 * 4 / 1e6
        print(f"rows {rows} ({mb:.0f} MB of state read per launch, as much again written at position 7)")
        for g in grids:
            med = [sorted(x)[len(x) // 2] for x in res[g]]
            ro = sum(med[:7]) / 7
            print(f"  n_wg {g:4d}{' (one workgroup per head)' if g == 0 else '':26s} read-only {ro:7.1f} us = {mb / ro:5.2f} TB/s"
                  f"   write-back {med[7]:7.1f} us = {2 * mb / med[7]:5.2f} TB/s   mean of 8 {sum(med) / 8:7.1f}   by position "
                  + " ".join(f"{m:.1f}" for m in med), flush=True)
        del c
        torch.cuda.empty_cache()


def sweep_loop(grids, passes, configs, steps=150):
    from lina_speech_amd.configs import l169
    from lina_speech_amd.decode import DecodeEngine, DecodeEngineGroup
    torch.manual_seed(0)
    m = l169().eval().to("cuda", torch.bfloat16)
    print(f"== greedy device loop, ms per token ({steps} steps per timing, median of passes | min .. max)")
    for n_eng, rows in configs:
        x = torch.randint(3, 256, (rows, 24), generator=torch.Generator().manual_seed(3)).cuda()
        with torch.inference_mode():
            xe = m.txt_encoder(m.txt_embed(x))
            engs = {}
            for g in grids:
                e = (DecodeEngineGroup(m, xe, batch_size=rows, n_engines=2, k1w_persist_wg=g) if n_eng == 2
                     else DecodeEngine(m, xe, batch_size=rows, k1w_persist_wg=g))
                e.begin_greedy(steps * (passes + 1) + 64, log_att=True)
                e.greedy_steps(24)
                engs[g] = e
            torch.cuda.synchronize()
            res = {g: [] for g in grids}
            for _ in range(passes):
                for g in grids:
                    engs[g].greedy_steps(8)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    engs[g].greedy_steps(steps)
                    torch.cuda.synchronize()
                    res[g].append((time.perf_counter() - t0) / steps * 1e3)
            name = f"{n_eng} x {rows // n_eng} rows" if n_eng == 2 else f"1 x {rows} rows"
            for g in grids:
                t = sorted(res[g])
                print(f"  {name:14s} n_wg {g:4d}  {t[len(t) // 2]:.4f} ms | {t[0]:.4f} .. {t[-1]:.4f}   {rows / t[len(t) // 2]:8.1f} k tok/s",
                      flush=True)
            for e in engs.values():
                e.close()
            del engs
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--grids", default="128,160,192,224,256")
    ap.add_argument("--loops", default="2x512,2x384,1x512,1x256,1x64", help="engines x total rows of the loop timings")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-loop", action="store_true")
    a = ap.parse_args()
    grids = [0] + [int(g) for g in a.grids.split(",") if g]
    ops.get_backend().lib
    print(torch.cuda.get_device_name(0), "| torch", torch.__version__)
    settle()
    if not a.skip_kernel:
        sweep_kernel(grids, a.passes)
    if not a.skip_loop:
        sweep_loop(grids, a.passes, [tuple(int(v) for v in c.split("x")) for c in a.loops.split(",")])


if __name__ == "__main__":
    main()
