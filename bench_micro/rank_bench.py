"""Times cudf::rank next to cudf::sorted_order of the same column, on 100M-row columns with 1M distinct values:
  I: int64, no nulls;   IN: int64, 10 % nulls (two-word plan);   F: float64, no nulls;   FN: float64, 10 % nulls (two-word plan).
For every column: sorted_order, then rank for each method without and with percentage (ascending, nulls after; EXCLUDE, so the
null columns copy their mask too).
usage: python bench_micro/rank_bench.py [rows] [columns I,IN,F,FN] [reps] [output file] [distinct]
Times are HIP events on the stream around the whole call (its read-backs included) after two warm-up calls, median of `reps`.
Per call: median ms; for rank also the time over sorted_order ("pass" = rank - sorted_order, the rank pass with its output
allocation and, for a null column, the mask copy), the rank kernels' own time from one profiled call, the time of the word fills
beyond sorted_order's (the two-word plan's refill), and the bandwidth of the rank kernels on the algorithmic bytes: per row 8 B
of words per plan word and 4 B of order read (FIRST: the order alone; DENSE reads the words twice), and 4 B (INT32) or 8 B
(FLOAT64) written scattered."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import cudf_amd
from bench_configs import bernoulli_mask
from cudf_amd import _lib
from cudf_amd import sorting as S
from cudf_amd.aggregation import RankMethod
from cudf_amd.types import NullOrder, NullPolicy, Order

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
columns = (sys.argv[2] if len(sys.argv) > 2 else "I,IN,F,FN").split(",")
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
out_path = sys.argv[4] if len(sys.argv) > 4 else None
distinct = int(sys.argv[5]) if len(sys.argv) > 5 else 1_000_000
dev = torch.device("cuda", 0)
lines = []
RANK_KERNELS = ("rank_first", "rank_ties", "rank_dense_count", "rank_dense_apply")


def say(line):
    print(line, flush=True)
    lines.append(line)


def median_ms(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def profiled(fn):
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    return _lib.profile_report()


def make(name):
    g = torch.Generator(device=dev).manual_seed(23)
    k = torch.randint(-distinct // 2, distinct - distinct // 2, (n,), device=dev, dtype=torch.int64, generator=g)
    if name.startswith("F"):
        k = k.to(torch.float64) / 8.0
    if name.endswith("N"):
        mask, nulls, _ = bernoulli_mask(n, 0.10, 29, dev)
        return cudf_amd.Column.from_torch(k, mask, nulls), k, 2
    return cudf_amd.Column.from_torch(k), k, 1


def algorithmic_bytes(method, nwords, as_double):
    words = 0 if method == RankMethod.FIRST else 8 * nwords * (2 if method == RankMethod.DENSE else 1)
    return n * (words + 4 + (8 if as_double else 4))


say(f"rank_bench rows={n} distinct={distinct} reps={reps} device={torch.cuda.get_device_name(0)}")
for name in columns:
    col, keep, nwords = make(name)
    t = cudf_amd.Table([col])
    order = lambda: S.sorted_order(t, [Order.ASCENDING], [NullOrder.AFTER])
    base = median_ms(order)
    prof = profiled(order)
    fills_ms = prof["sort_pack_words"][1]
    say(f"{name:2s} {'sorted_order':18s} {base:8.2f} ms  fills={prof.get('sort_pack_words', (0, 0))[0]} ({fills_ms:.2f} ms) "
        f"passes={prof.get('sort_scatter', (0, 0))[0]}")
    for method in RankMethod:
        for pct in (False, True):
            fn = lambda: S.rank(col, method, Order.ASCENDING, NullPolicy.EXCLUDE, NullOrder.AFTER, pct)
            ms = median_ms(fn)
            prof = profiled(fn)
            kernel_ms = sum(prof[k][1] for k in RANK_KERNELS if k in prof)
            refill_ms = prof["sort_pack_words"][1] - fills_ms  # (the fills beyond sorted_order's: the two-word plan's value word)
            scan_ms = prof["sort_scan"][1] / prof["sort_scan"][0] if method == RankMethod.DENSE else 0.0
            gbs = algorithmic_bytes(method, nwords, pct or method == RankMethod.AVERAGE) / kernel_ms / 1e6
            ran = " ".join(f"{k}={prof[k][0]}" for k in RANK_KERNELS if k in prof)
            say(f"{name:2s} {method.name.lower() + ('_pct' if pct else ''):18s} {ms:8.2f} ms  pass={ms - base:7.2f} ms  "
                f"rank kernels={kernel_ms:6.2f} ms ({gbs:6.0f} GB/s)  refill={refill_ms:5.2f} ms  scan~{scan_ms:5.2f} ms  [{ran}]")
    del col, keep, t
    torch.cuda.empty_cache()
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
