"""K14 (cross-entropy) forward: time per call of ``ops.cross_entropy`` at the codec head's shapes.

    python tools/perf_k14.py                       # the in-tree library
    python tools/perf_k14.py before=/path/to/other/liblina_gla.so

Every ``name=path`` names another build of the C ABI (e.g. one linked with an earlier csrc/train_fused.hip); the libraries
are timed interleaved, 5 rounds of 20 calls after 3 warm-up calls each, and the mean loss of each is printed so that a change
of the summation shows.  The time covers the whole forward of ``ops.cross_entropy``: K14 plus the two K13 sums."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from lina_speech_amd import _lib, ops
from lina_speech_amd.backend import HipBackend


def main():
    dev = "cuda"
    paths = [("in-tree", _lib.LIB_PATH)] + [tuple(a.split("=", 1)) for a in sys.argv[1:]]
    libs = {}
    for name, path in paths:
        be = HipBackend()
        be._lib = _lib.bind(path)
        libs[name] = be
    g = torch.Generator().manual_seed(0)
    for N, V, dt in ((32768, 4099, torch.bfloat16), (32768, 4099, torch.float32), (4096, 1027, torch.bfloat16)):
        lg = (torch.randn(N, V, generator=g) * 4).to(dt).to(dev)
        tg = torch.randint(0, V, (N,), generator=g).to(dev)
        res, losses = {k: [] for k in libs}, {}
        for _ in range(5):
            for name, be in libs.items():
                ops.set_backend(be)
                for _ in range(3):
                    ops.cross_entropy(lg, tg, ignore_index=1)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    loss = ops.cross_entropy(lg, tg, ignore_index=1)
                e1.record()
                torch.cuda.synchronize()
                res[name].append(e0.elapsed_time(e1) / 20 * 1e3)
                losses[name] = float(loss)
        for name, v in res.items():
            print(f"{N} x {V} {str(dt).split('.')[-1]:9s} {name:10s} min {min(v):7.1f} us  median {sorted(v)[2]:7.1f} us  "
                  f"loss {losses[name]!r}", flush=True)


if __name__ == "__main__":
    main()
