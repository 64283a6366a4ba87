"""Times cudf::sorted_order and cudf::sort_by_key (one 8-byte payload column) on four 100M-row keys, next to torch.argsort(stable=True)
/ torch.sort of the same keys for the single-column ones, and prints the radix passes each call ran.
  K1: one int64 key, uniform over the whole range;
  K2: one float64 key, standard normal;
  K3: (int32, int32), both uniform over the whole range: one packed word, 8 passes;
  K4: (int64, nullable int32 descending, 10 % nulls): the int32 field in one word, the int64 in the next.
usage: python bench_micro/sorting_bench.py [rows] [keys K1,K2,K3,K4] [reps] [output file]
Times are HIP events on the stream around the whole call (its read-backs included) after two warm-up calls, median of `reps`.
Per key and call: median ms, the sort_pack_words / sort_scatter launches, and the per-kernel split of one profiled call."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import cudf_amd
from bench_configs import bernoulli_mask
from cudf_amd import _lib
from cudf_amd import sorting as S
from cudf_amd.types import NullOrder, Order

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
keys = (sys.argv[2] if len(sys.argv) > 2 else "K1,K2,K3,K4").split(",")
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
out_path = sys.argv[4] if len(sys.argv) > 4 else None
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


def make(key):
    g = torch.Generator(device=dev).manual_seed(17)
    col = cudf_amd.Column.from_torch
    if key == "K1":
        k = torch.randint(-2**63, 2**63 - 1, (n,), device=dev, dtype=torch.int64, generator=g)
        return [col(k)], [], [], k
    if key == "K2":
        k = torch.randn((n,), device=dev, dtype=torch.float64, generator=g)
        return [col(k)], [], [], k
    if key == "K3":
        a = torch.randint(-2**31, 2**31 - 1, (n,), device=dev, dtype=torch.int32, generator=g)
        b = torch.randint(-2**31, 2**31 - 1, (n,), device=dev, dtype=torch.int32, generator=g)
        return [col(a), col(b)], [], [], None
    a = torch.randint(-2**63, 2**63 - 1, (n,), device=dev, dtype=torch.int64, generator=g)
    b = torch.randint(-2**31, 2**31 - 1, (n,), device=dev, dtype=torch.int32, generator=g)
    mask, nulls, _ = bernoulli_mask(n, 0.10, 19, dev)
    return [col(a), col(b, mask, nulls)], [Order.ASCENDING, Order.DESCENDING], [NullOrder.BEFORE, NullOrder.BEFORE], None


say(f"sorting_bench rows={n} reps={reps} device={torch.cuda.get_device_name(0)}")
payload = cudf_amd.Table([cudf_amd.Column.from_torch(torch.arange(n, device=dev, dtype=torch.float64))])
for key in keys:
    cols, o, no, single = make(key)
    t = cudf_amd.Table(cols)
    calls = {"sorted_order": lambda: S.sorted_order(t, o, no), "sort_by_key+payload": lambda: S.sort_by_key(payload, t, o, no)}
    for name, fn in calls.items():
        ms = median_ms(fn)
        prof = profiled(fn)
        split = " ".join(f"{k}={v[1]:.2f}" for k, v in sorted(prof.items()))
        say(f"{key} {name:22s} {ms:8.2f} ms  {n / ms / 1e6:7.2f} G rows/s  fills={prof.get('sort_pack_words', (0, 0))[0]} "
            f"passes={prof.get('sort_scatter', (0, 0))[0]}  [{split}]")
    assert S.is_sorted(S.sort(t, o, no), o, no)
    if single is not None:
        say(f"{key} {'torch.argsort(stable)':22s} {median_ms(lambda: torch.argsort(single, stable=True)):8.2f} ms")
        say(f"{key} {'torch.sort':22s} {median_ms(lambda: torch.sort(single)):8.2f} ms")
    del cols, t, single
    torch.cuda.empty_cache()
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
