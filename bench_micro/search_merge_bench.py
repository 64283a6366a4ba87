"""Times cudf::lower_bound and cudf::merge on sorted int64 tables, and prints the kernels each call ran.
  S1: lower_bound of `needles` SORTED int64 needles in a `rows`-row sorted int64 haystack;
  S2: the same needles shuffled;
  M1: merge of two sorted tables of rows / 2 rows each (int64 key, one 8-byte payload), next to cudf::sort of the same `rows` rows
      concatenated on the host - the existing sort path a caller without merge has to run again.
usage: python bench_micro/search_merge_bench.py [rows] [needles] [reps] [output file]
       (defaults: 100M rows, 10M needles, 7 reps, profiles/search_merge_bench.txt)
Times are HIP events on the stream around the whole call (its read-backs included) after two warm-up calls, median of `reps`.
Per call: median ms and the per-kernel split of one profiled call."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import cudf_amd
from cudf_amd import _lib
from cudf_amd import merge as M
from cudf_amd import search, sorting
from cudf_amd.types import Order

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
needles_n = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "search_merge_bench.txt")
dev = torch.device("cuda", 0)
lines = []


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


def report(name, rows, fn):
    ms = median_ms(fn)
    split = " ".join(f"{k}={v[0]}x{v[1]:.2f}" for k, v in sorted(profiled(fn).items()))
    say(f"{name:28s} {ms:8.2f} ms  {rows / ms / 1e6:7.2f} G rows/s  [{split}]")


col = cudf_amd.Column.from_torch
g = torch.Generator(device=dev).manual_seed(23)
say(f"search_merge_bench rows={n} needles={needles_n} reps={reps} device={torch.cuda.get_device_name(0)}")

# ---- S1 / S2
hay = torch.sort(torch.randint(-2**62, 2**62, (n,), device=dev, dtype=torch.int64, generator=g)).values
shuffled = torch.randint(-2**62, 2**62, (needles_n,), device=dev, dtype=torch.int64, generator=g)
ordered = torch.sort(shuffled).values
h = cudf_amd.Table([col(hay)])
for name, needles in (("S1 lower_bound sorted", ordered), ("S2 lower_bound shuffled", shuffled)):
    t = cudf_amd.Table([col(needles)])
    report(name, needles_n, lambda: search.lower_bound(h, t))
    assert torch.equal(search.lower_bound(h, t).to_torch().to(torch.int64), torch.searchsorted(hay, needles))
del hay, shuffled, ordered, h, t
torch.cuda.empty_cache()

# ---- M1
half = n // 2
keys = [torch.sort(torch.randint(-2**62, 2**62, (half,), device=dev, dtype=torch.int64, generator=g)).values for _ in range(2)]
pays = [torch.arange(half, device=dev, dtype=torch.int64) + (i << 32) for i in range(2)]
tables = [cudf_amd.Table([col(k), col(p)]) for k, p in zip(keys, pays)]
report("M1 merge 2 sorted tables", 2 * half, lambda: M.merge(tables, [0], [Order.ASCENDING]))
merged = M.merge(tables, [0], [Order.ASCENDING])
assert sorting.is_sorted(cudf_amd.Table([merged.columns()[0]]), [Order.ASCENDING], [])
del merged
both = cudf_amd.Table([col(torch.cat(keys).cpu().to(dev)), col(torch.cat(pays).cpu().to(dev))])  # concatenated on the host
key_view = cudf_amd.Table([both.columns()[0]])
report("M1 sort_by_key of all rows", 2 * half, lambda: sorting.sort_by_key(both, key_view))

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
