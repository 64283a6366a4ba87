"""Times cudf::distinct_count, distinct_indices (KEEP_FIRST, KEEP_NONE) and stable_distinct (KEEP_ANY, with the payload) on three
100M-row shapes, next to torch.unique of the same keys and the library's own groupby COUNT_ALL, and checks every count against
torch.unique.
  D1: int64 keys uniform over [0, 1M) (dense form) + one float64 payload column;
  D2: int64 keys drawn from 50M random 64-bit values, about 43M distinct (hash set, inline keys) + the payload;
  D3: C4's keys, int64 in [0, 10^4) and int32 in [0, 10^3) with 10 % nulls, nulls EQUAL (hash set, {hash | row} slots) + payload.
usage: python bench_micro/distinct_bench.py [rows] [shapes D1,D2,D3] [reps]
Prints per shape and call: median ms, and the share of the 8 TB/s peak that the algorithmic bytes take."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C

import torch

import cudf_amd
from bench_configs import bernoulli_mask
from cudf_amd import _lib, reduce
from cudf_amd import aggregation as agg
from cudf_amd import groupby as gb
from cudf_amd import stream_compaction as SC
from cudf_amd.types import DuplicateKeepOption as K
from cudf_amd.types import NullPolicy

PEAK = 8e12
n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
shapes = (sys.argv[2] if len(sys.argv) > 2 else "D1,D2,D3").split(",")
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
lib = _lib.load()
dev = torch.device("cuda", 0)


def median_ms(fn):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return sorted(times)[len(times) // 2]


def profile(fn):
    lib.cudf_amd_profile_enable(1)
    lib.cudf_amd_profile_reset()
    fn()
    torch.cuda.synchronize()
    buf = C.create_string_buffer(1 << 16)
    lib.cudf_amd_profile_report(buf, len(buf))
    lib.cudf_amd_profile_enable(0)
    return " ".join(f"{ln.split()[0]}={float(ln.split()[2]):.2f}" for ln in buf.value.decode().splitlines())


def report(shape, name, ms, bytes_, extra=""):
    print(f"{shape} {name:28s} {ms:8.2f} ms  {bytes_ / 1e9:6.2f} GB  {bytes_ / (ms * 1e-3) / PEAK * 100:5.1f} % of peak  {extra}", flush=True)


g = torch.Generator(device=dev).manual_seed(5)
payload = cudf_amd.Column.from_torch(torch.rand(n, generator=g, device=dev, dtype=torch.float64))
for shape in shapes:
    if shape == "D1":
        k = torch.randint(0, 1_000_000, (n,), generator=g, device=dev, dtype=torch.int64)
        keys = [cudf_amd.Column.from_torch(k)]
        key_bytes = 8.0
        expect = torch.unique(k).numel()
    elif shape == "D2":
        pool = torch.randint(-2**62, 2**62, (50_000_000,), generator=g, device=dev, dtype=torch.int64)
        k = pool[torch.randint(0, pool.numel(), (n,), generator=g, device=dev)]
        del pool
        keys = [cudf_amd.Column.from_torch(k)]
        key_bytes = 8.0
        expect = torch.unique(k).numel()
    else:
        k = torch.randint(0, 10_000, (n,), generator=g, device=dev, dtype=torch.int64)
        k1 = torch.randint(0, 1_000, (n,), generator=g, device=dev, dtype=torch.int32)
        k1m, k1nulls, k1valid = bernoulli_mask(n, 0.10, 47, dev)
        keys = [cudf_amd.Column.from_torch(k), cudf_amd.Column.from_torch(k1, k1m, k1nulls)]
        key_bytes = 12 + 1 / 8
        combo = torch.where(k1valid, k * 1000 + k1.to(torch.int64), -1 - k)  # a NULL k1: one key per k0 (nulls EQUAL)
        expect = torch.unique(combo).numel()
        del combo
    kt = cudf_amd.Table(keys)
    full = cudf_amd.Table(keys + [payload])
    got = reduce.distinct_count_table(kt)
    print(f"{shape} rows {n} distinct {got} torch.unique {expect} count_ok {got == expect}", flush=True)
    # the algorithmic bytes: every key read once, the n-bit survivor mask written and read, the output indices written
    ms = median_ms(lambda: reduce.distinct_count_table(kt))
    report(shape, "distinct_count", ms, n * key_bytes, f"[{profile(lambda: reduce.distinct_count_table(kt))}]")
    for keep in (K.KEEP_FIRST, K.KEEP_NONE):
        idx = SC.distinct_indices(kt, keep)
        m = idx.size()
        ok = m == expect if keep == K.KEEP_FIRST else m <= expect
        del idx
        ms = median_ms(lambda: SC.distinct_indices(kt, keep))
        report(shape, f"distinct_indices({keep.name})", ms, n * (key_bytes + 2 / 8) + 4 * m,
               f"rows {m} ok {ok} [{profile(lambda: SC.distinct_indices(kt, keep))}]")
    out = SC.stable_distinct(full, list(range(len(keys))), K.KEEP_ANY)
    m = out.num_rows()
    del out
    ms = median_ms(lambda: SC.stable_distinct(full, list(range(len(keys))), K.KEEP_ANY))
    report(shape, "stable_distinct(KEEP_ANY)+pay", ms, n * (key_bytes + 2 / 8) + m * (4 + 2 * (key_bytes + 8)), f"rows {m} ok {m == expect}")
    if shape in ("D1", "D2"):
        ms = median_ms(lambda: torch.unique(k))
        report(shape, "torch.unique", ms, n * key_bytes)
    if shape == "D1":
        def gby():
            grp = gb.GroupBy(kt, NullPolicy.INCLUDE)
            return grp.aggregate([gb.GroupByRequest(payload, [agg.count(NullPolicy.INCLUDE)])])
        ms = median_ms(gby)
        report(shape, "groupby COUNT_ALL", ms, n * (key_bytes + 8))
    del kt, full, keys, k
    torch.cuda.empty_cache()
