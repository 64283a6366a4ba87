"""Times cudf::apply_boolean_mask on 1, 2 and 4 float64 columns, with and without null masks, at selectivities 0.001, 0.5 and
0.999, and prints the kernels each call ran. Beside each line: torch's boolean indexing x[mask] of the same columns on the same
device, an outside yardstick (it moves no validity).
usage: python bench_micro/copy_if_bench.py [rows ...] [--reps R] [--out FILE]
       (defaults: 100M and 500M rows, 7 reps, profiles/copy_if_bench.txt)
Times are HIP events on the stream around the whole call (its read-backs included) after two warm-up calls, median of `reps`.
GB/s is on the algorithmic bytes of DESIGN.md section 4, "Filtering rows": the boolean column read once (n), the selection words
written and read (2 n / 8), per column 8 n s bytes read and 8 n s written, per nullable column n / 8 validity bytes read and
n s / 8 written."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import cudf_amd
from cudf_amd import _lib
from cudf_amd import stream_compaction as SC
from cudf_amd.types import DataType, TypeId

args = sys.argv[1:]
reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 7
out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "copy_if_bench.txt")
sizes = [int(a) for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or not args[i - 1].startswith("--"))]
sizes = sizes or [100_000_000, 500_000_000]
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


g = torch.Generator(device=dev).manual_seed(29)
say(f"copy_if_bench rows={sizes} reps={reps} device={torch.cuda.get_device_name(0)}")
for n in sizes:
    data = [torch.rand(n, device=dev, dtype=torch.float64, generator=g) for _ in range(4)]
    words = (n + 31) // 32
    valid = [torch.randint(-2**31, 2**31, (words + 16,), device=dev, dtype=torch.int32, generator=g) for _ in range(4)]
    for s in (0.001, 0.5, 0.999):
        m = torch.rand(n, device=dev, generator=g) < s
        mask = cudf_amd.Column.from_torch(m.view(torch.uint8), dtype=DataType(TypeId.BOOL8))
        kept = int(m.sum())
        for ncols in (1, 2, 4):
            for nulls in (False, True):
                cols = [cudf_amd.Column.from_torch(d, v if nulls else None, null_count=1 if nulls else 0)
                        for d, v in zip(data[:ncols], valid)]
                t = cudf_amd.Table(cols)
                fn = lambda: SC.apply_boolean_mask(t, mask)
                assert fn().num_rows() == kept
                ms = median_ms(fn)
                nbytes = n + 2 * n / 8 + ncols * 16 * kept + (ncols * (n / 8 + kept / 8) if nulls else 0)
                split = " ".join(f"{k}={v[0]}x{v[1]:.2f}" for k, v in sorted(profiled(fn).items()))
                t_ms = median_ms(lambda: [d[m] for d in data[:ncols]])
                say(f"n={n} s={s} cols={ncols} nulls={int(nulls)}: {ms:8.2f} ms {nbytes / ms / 1e6:8.1f} GB/s | torch x[mask] "
                    f"{t_ms:8.2f} ms [{split}]")
        del m, mask
    del data, valid
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
