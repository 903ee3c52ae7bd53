#!/usr/bin/env python
"""K1w by WINDOW POSITION and the overlap of the two engines' streams, from a rocprofv3 (rocpd sqlite) kernel trace of
`bench.py --steps 300 --warmup 16 --full --headline-only` (two engines; once more with `--engines 1`):

  (a) K1w duration by window position, per launch grid: the K1w launches of one queue come layer by layer, token by token, so
      launch i of a queue is layer i % L of token i // L, and every W-th token writes the state back; the phase of the window
      is taken from the data (the position with the longest mean).  Mean / p5 / p95, and the kernel's registers / LDS as loaded.
  (b) per token: the time in which a K1w of one queue and another kernel (the "chain") of the other queue are both
      executing, K1w || K1w, chain || chain, and one queue only.
      (On this stack the traced run SERIALISES the streams -- the figures then only prove that, and the tool says so.)

    python tools/prof_overlap.py <results.db> [out.txt] [--layers 13] [--window 8] [--tokens N]"""
import argparse
import sqlite3


def pct(v, p):
    v = sorted(v)
    return v[min(len(v) - 1, int(p / 100 * len(v)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("out", nargs="?")
    ap.add_argument("--layers", type=int, default=13, help="K1w launches per token and engine (L169: 6 + 6 + pos_net)")
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--gap-ms", type=float, default=5.0, help="a pause between K1w launches of a queue that ends a run")
    ap.add_argument("--tokens", type=int, default=0,
                    help="tokens per engine the overlap figures are divided by (default: the first queue's K1w launches / layers)")
    a = ap.parse_args()
    cur = sqlite3.connect(a.db).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)").fetchall()]
    pick = lambda *names: next((n for n in names if n in cols), None)
    # the HIP STREAM, not the hardware queue: the runtime spreads one stream's graph launches over several hardware queues
    q = pick("stream_id", "stream", "queue_id", "queue")
    extra = [c for c in (pick("arch_vgpr_count", "vgpr_count"), pick("accum_vgpr_count"), pick("lds_size", "lds_block_size"),
                         pick("scratch_size")) if c]
    sel = ", ".join(["name", "start", "end", "grid_x", "workgroup_x", q or "0"] + extra)
    rows = cur.execute(f"select {sel} from kernels order by start").fetchall()
    lines = [f"streams by `{q}`: " + ", ".join(f"{k}: {n} launches" for k, n in cur.execute(
        f"select {q or 0}, count(*) from kernels group by 1 order by 2 desc").fetchall()[:6])]
    is_k1w = lambda n: "gla_decode_window" in n
    if "stream_id" in cols and "queue_id" in cols:
        lines.append("K1w launches by (stream_id, queue_id): " + ", ".join(f"({x}, {y}): {n}" for x, y, n in cur.execute(
            "select stream_id, queue_id, count(*) from kernels where name like '%gla_decode_window%' group by 1, 2 order by 3 desc").fetchall()[:8]))
    # ---- (a)
    # a queue's K1w launches, cut into RUNS at pauses of more than --gap-ms (graph replays of one greedy_steps call follow
    # each other closely -- under the profiler every replay of the 8-token graph is a run of its own; the flush launches of the
    # same kernel at a state read-out come after a pause and make short runs, which are dropped)
    by = {}
    for r in rows:
        if is_k1w(r[0]):
            by.setdefault((r[5], r[3] // max(r[4], 1), r[0].split("(")[0].replace("void lina::", "")[:60], tuple(r[6:])), []).append(r)
    lines.append(f"(a) K1w by window position (W = {a.window}, {a.layers} launches per token, runs of >= {a.window} tokens); us: mean / p5 / p95")
    for (queue, wgs, name, res), rr in sorted(by.items(), key=lambda kv: (kv[0][1], str(kv[0][0]))):
        runs, cur_run = [], [rr[0]]
        for prev, r in zip(rr, rr[1:]):
            if r[1] - prev[2] > a.gap_ms * 1e6:
                runs.append(cur_run)
                cur_run = []
            cur_run.append(r)
        runs.append(cur_run)
        pos = [[] for _ in range(a.window)]
        n_used = 0
        for run in runs:
            d = [(r[2] - r[1]) / 1e3 for r in run]
            n_tok = len(d) // a.layers
            if n_tok < a.window:
                continue
            p = [[] for _ in range(a.window)]
            for i, x in enumerate(d[:n_tok * a.layers]):
                p[(i // a.layers) % a.window].append(x)
            wb = max(range(a.window), key=lambda j: sum(p[j]) / len(p[j]))      # the run's phase: from the data
            for j in range(a.window):
                pos[j] += p[(wb + 1 + j) % a.window]
            n_used += n_tok * a.layers
        if not n_used:
            continue
        lines.append(f"  stream {queue}  {wgs} workgroups  {name}  " + " ".join(f"{c}={v}" for c, v in zip(extra, res))
                     + f"  ({n_used} of {len(rr)} launches in {len(runs)} runs)")
        for j in range(a.window):
            p = pos[j]
            lines.append(f"    position {j}{' (write-back)' if j == a.window - 1 else '':13s} {sum(p) / len(p):8.1f} / {pct(p, 5):8.1f} / {pct(p, 95):8.1f}")
        ro = [x for j in range(a.window - 1) for x in pos[j]]
        lines.append(f"    write-back / read-only mean = {sum(pos[-1]) / len(pos[-1]) / (sum(ro) / len(ro)):.2f}")
    # ---- (b): sweep over the start / end events of the two busiest queues
    queues = {}
    for r in rows:
        queues[r[5]] = queues.get(r[5], 0) + is_k1w(r[0])
    top = sorted(queues, key=queues.get, reverse=True)[:2]
    if len(top) == 2 and queues[top[1]] > 0:
        ev = []
        for r in rows:
            if r[5] in top:
                k = (top.index(r[5]), is_k1w(r[0]))
                ev += [(r[1], 1, k), (r[2], -1, k)]
        ev.sort(key=lambda e: (e[0], e[1]))
        live = {(s, w): 0 for s in (0, 1) for w in (False, True)}
        acc = {"K1w || chain": 0, "K1w || K1w": 0, "chain || chain": 0, "one stream only": 0, "idle": 0}
        t_prev = ev[0][0]
        for t, d, k in ev:
            dt = t - t_prev
            s = [live[(i, True)] > 0 for i in (0, 1)], [live[(i, False)] > 0 for i in (0, 1)]
            busy = [s[0][i] or s[1][i] for i in (0, 1)]
            if busy[0] and busy[1]:
                if s[0][0] and s[0][1]:
                    acc["K1w || K1w"] += dt
                elif s[0][0] or s[0][1]:
                    acc["K1w || chain"] += dt
                else:
                    acc["chain || chain"] += dt
            elif busy[0] or busy[1]:
                acc["one stream only"] += dt
            else:
                acc["idle"] += dt
            live[k] += d
            t_prev = t
        n_tok = a.tokens or max(1, queues[top[0]] // a.layers)
        lines.append(f"(b) two streams ({top[0]}, {top[1]}), us per token over the {n_tok} tokens of the trace (pre-heat and warm-up included):")
        for k, v in acc.items():
            lines.append(f"    {k:16s} {v / 1e3 / n_tok:9.1f}")
        both = acc["K1w || chain"] + acc["K1w || K1w"] + acc["chain || chain"]
        if both < 0.1 * acc["one stream only"]:
            lines.append("    -> the streams overlap in under a tenth of their busy time: this trace was taken with the kernels SERIALISED "
                         "(the profiler's dispatch interception), so it says what each launch costs ALONE, not what runs beside what")
    else:
        lines.append("(b) one stream with K1w launches: no overlap to report")
    # chain launches: mean duration of the most frequent non-K1w kernels
    chain = {}
    for r in rows:
        if not is_k1w(r[0]):
            chain.setdefault(r[0].split("(")[0].replace("void lina::", "")[:70], []).append((r[2] - r[1]) / 1e3)
    lines.append("chain kernels, mean us (launches):")
    for n, d in sorted(chain.items(), key=lambda kv: -sum(kv[1]))[:12]:
        lines.append(f"    {n:70s} {sum(d) / len(d):8.2f} ({len(d)})")
    out = "\n".join(lines)
    print(out)
    if a.out:
        open(a.out, "w").write(out + "\n")


if __name__ == "__main__":
    main()
