#!/usr/bin/env python
"""Kernel time of the keywords of DESIGN.md section 6j, off and on, at V = 32000 and 1 and 64 rows: the one-sequence sampler
(sample_kernel), the per-row tail (sample_rows_kernel) and the processor filter (logits_process_kernel) through their op-level calls.
    python tools/bench_warpers.py off|on [iterations]
off: T 0.7, top_k 50, top_p 0.9; repetition penalty 1.3 over histories of 128 ids.
on : the same plus min_p 0.05, typical_p 0.9, epsilon_cutoff 3e-4, eta_cutoff 6e-4; plus 32 sequences of up to 8 ids (16 biases, 16 bad words).
Prints the mean time per launch between two events; under `rocprofv3 --kernel-trace --stats` the kernels' own durations are in the trace
(tools/bench_warpers.py summarise <kernel_trace.csv> prints them per kernel and grid)."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vision-zephyr_amd"))


def summarise(path):
    import collections
    import csv
    d = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        n = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "")
        if any(k in n for k in ("sample_kernel", "sample_rows_kernel", "logits_process_kernel")):
            d[(n[:48], int(r["Grid_Size_X"]) // 1024)].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    for (n, rows), v in sorted(d.items()):
        v = sorted(v)[: max(1, len(v) - len(v) // 10)]          # without the slowest tenth (first launches)
        print(f"{n:48s} rows {rows:3d}: {len(v):5d} launches, mean {sum(v) / len(v) / 1e3:8.2f} us, min {v[0] / 1e3:8.2f} us")


def main():
    import torch
    from vz_hip import binding as B
    from vz_hip.logits_proc import ProcConfig
    from vz_hip.sample_rows import RowParams
    on = sys.argv[1] == "on"
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    V = 32000
    g = torch.Generator().manual_seed(1)
    warp = dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=6e-4) if on else {}
    seq = tuple(((100 + i, 200 + i, 300 + i, 400 + i, 500 + i, 600 + i, 700 + i, 800 + i)[: 1 + i % 8], 0.5 * i, False) for i in range(16)) + \
        tuple(((900 + i, 1000 + i, 1100 + i)[: 1 + i % 3], float("-inf"), True) for i in range(16))
    cfg = ProcConfig(penalty=1.3, seq=seq if on else ())

    def timed(name, fn):
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        print(f"{sys.argv[1]:3s} {name:34s}: {a.elapsed_time(b) / iters * 1e3:8.2f} us per call (host launch included)")

    for rows in (1, 64):
        x = (torch.randn(rows, V, generator=g) * 2.5).float().cuda()
        p = RowParams(True, 0.7, 50, 0.9, 7, 0, **warp)
        params = [p] * rows
        hist = torch.randint(0, V, (rows, 128), generator=g, dtype=torch.int32).cuda()
        hl = torch.full((rows,), 128, dtype=torch.int32).cuda()
        y = x.clone()
        timed(f"sample_kernel rows {rows}", lambda: B.sample(x, 0.7, 50, 0.9, 7, 0, warp=p.warp))
        timed(f"sample_rows_kernel rows {rows}", lambda: B.sample_rows(x, params))
        timed(f"logits_process_kernel rows {rows}", lambda: B.logits_process(y, cfg, hist, hl))


if __name__ == "__main__":
    if sys.argv[1] == "summarise":
        summarise(sys.argv[2])
    else:
        main()
